// frame_settings.h — the frame settings of a matcher as ONE record (include/slideo_amd.h "Working size", "Frame region", "Frame mask",
// "Frame mask scope", "Direct page look-up", "Direct look-up scope", "YUV colour description", "YUV sampling", "YUV chroma filter", "YUV transfer", "Gate reference", "Gate settle", "Gate memory", "Frame pixel format", "Frame levels", "Frame shading", "Frame lens"): the record, every setter's proposal with its range checks, the
// rules between settings, what a change of each ends.  Plain C++, no HIP include (tools/frame_settings_hostcheck.cpp walks it on the
// host); the device buffers a setting owns are the matcher's (runtime.hpp); the frame
// shading's nodes are the record's own, shared by pointer between its copies.  A change takes ONE path: settings_commit (capi_runtime.hip).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "error.h"
#include "geom.h"

namespace slideo {

// The region's 3x3 map M from the rectified out_w x out_h image into source frames of src_w x src_h, and the rectify_kernel instance
// the host chose from M (frame_region.hip.h RECT_*; tx, ty: RECT_TRANSLATE)
struct FrameRegion {
    bool set = false;
    int src_w = 0, src_h = 0, out_w = 0, out_h = 0;
    double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int kind = 0, tx = 0, ty = 0;
};
// The radial lens of "Frame lens": a point p of the ideal source plane is seen at c + (p - c) g(r2), r2 = |p - c|^2 / f^2, g = 1 + k1 r2 +
// k2 r2^2; q = 1.0 / (f * f), computed once at the proposal.  set false: off, and k1 == k2 == 0 is stored as off
struct FrameLens {
    bool set = false;
    int src_w = 0, src_h = 0;
    double cx = 0, cy = 0, f = 0, k1 = 0, k2 = 0, q = 0;
};
// A w x h mask; frames of that analysed size keep only the FAST candidates its pyramid (the matcher's d_mask_pyr) allows
struct FrameMask { bool set = false; int w = 0, h = 0; };
// The gate's validity map, in force while a mask is set under SLIDEO_MASK_GATE: one weight byte (0xFF valid, 0x00) per byte of the
// sw x sh small image of frames of the mask's size (the matcher's d_gate_w), n_valid valid pixels
struct GateMap { bool on = false; int sw = 0, sh = 0; int64_t n_valid = 0; };

// How every slideo_yuv420_layout call reads its samples (SLIDEO_YUV_MATRIX_* / _RANGE_* / _DEPTH_*); all 0: the default.  The
// sampling (SLIDEO_YUV_SAMPLING_*, "YUV sampling") is set on its own and says where the samples lie.
// The chroma filter (SLIDEO_YUV_CHROMA_*, "YUV chroma filter") is set on its own too and says how a pixel's chroma is read from them
struct YuvDesc {
    int matrix = SLIDEO_YUV_MATRIX_BT601, range = SLIDEO_YUV_RANGE_LIMITED, depth = SLIDEO_YUV_DEPTH_8;
    int sampling = SLIDEO_YUV_SAMPLING_420;
    int chroma = SLIDEO_YUV_CHROMA_NEAREST;
    // the transfer (SLIDEO_YUV_TRANSFER_*, "YUV transfer") is set on its own as well; white_nits: the display light that becomes SDR
    // white, as resolved (0 under SDR; a set call's 0 is stored as 203).  The matcher's d_transfer holds the tables' device copy
    int transfer = SLIDEO_YUV_TRANSFER_SDR;
    float white_nits = 0.f;
    // the bilinear kernel converts the frames: a filter is set and the sampling has chroma to interpolate
    bool filtered() const { return chroma != SLIDEO_YUV_CHROMA_NEAREST && sampling != SLIDEO_YUV_SAMPLING_444; }
    int bytes_per_sample() const { return depth == SLIDEO_YUV_DEPTH_8 ? 1 : 2; }
};
// The per-channel tone table of "Frame levels": lut[c * 256 + v], c = 0, 1, 2 for B, G, R (the matcher's d_levels holds its copy on
// the device); set false: off, and the identity table is stored as off
struct FrameLevels { bool set = false; uint8_t lut[768] = {}; };
// The gain field of "Frame shading": Q8.8 nodes gains[j * (gw + 1) + i] at pixel (i * cell, j * cell) of the aw x ah analysed image,
// gw = ceil(aw / cell), gh = ceil(ah / cell) (the matcher's d_shading holds their copy on the device); set false: off, and the
// all-256 field is stored as off.  The nodes are shared by every copy of the record, never written after the proposal
struct FrameShading {
    bool set = false;
    int aw = 0, ah = 0, cell = 0;
    std::shared_ptr<const std::vector<uint16_t>> gains;
    int gw() const { return (aw + cell - 1) / cell; }
    int gh() const { return (ah + cell - 1) / cell; }
};

struct FrameSettings {
    int work_w = 0, work_h = 0;                       // frames beyond it are reduced in front of the pipeline; 0, 0 = none
    FrameRegion region;                               // frames of region.src_w x src_h stand for their rectified image
    FrameLens lens;                                   // frames of lens.src_w x src_h are undistorted in the rectify's launch
    FrameMask mask;
    uint32_t mask_scope = SLIDEO_MASK_DETECT;         // SLIDEO_MASK_DETECT | SLIDEO_MASK_GATE; the matcher's, whatever happens to the mask
    GateMap gate_map;
    uint64_t gate_map_gen = 1;                        // what is derived from the map (the look-up's masked page norms) is cached under it
    float direct_t = 0.f;                             // the direct similarity (0: off)
    uint32_t direct_scope = SLIDEO_DIRECT_WHOLE;      // VALID = the look-up over the gate's valid pixels
    YuvDesc yuv;                                      // 4:2:0 frames stand for the BGR image under it (BGR calls never look at it)
    int pixel_format = SLIDEO_PIXEL_BGR8;             // how every *_bgr8 frame call reads its frames (YUV calls never look at it)
    FrameShading shading;                             // the unit's BGR image is multiplied by it, in front of the levels
    FrameLevels levels;                               // the unit's BGR image goes through it, the last step in front of the unit
    uint32_t gate_ref = SLIDEO_GATE_PREVIOUS;         // what a gated frame is compared with: the frame before it, or the last changed one (ANCHOR)
    // the gate settle, part of the gate-reference setting ("Gate settle"): under ANCHOR a frame away from the anchor is matched once it
    // is within settle_similarity of the frame before it, or after settle_max_defer deferred frames; 0: off
    float settle_similarity = 0.f;
    int32_t settle_max_defer = 0;
    // the gate memory, part of the gate-reference setting ("Gate memory"): under ANCHOR the last gate_memory matched frames are kept
    // and a frame away from the anchor that is within changed_similarity of one of them is recalled, not matched; 0: off
    int32_t gate_memory = 0;
    bool gate_scope() const { return mask.set && (mask_scope & SLIDEO_MASK_GATE); }      // the gate compares under the mask
};

enum Setting { SET_WORKING_SIZE, SET_FRAME_REGION, SET_FRAME_MASK, SET_FRAME_MASK_SCOPE, SET_DIRECT_SIMILARITY, SET_DIRECT_SCOPE, SET_YUV_DESCRIPTION,
               SET_GATE_REFERENCE, N_SETTINGS };

// What a change of each setting ends: the frames a mask call kept (made under the earlier setting), the gate state (so was its small
// image; under a mask change it stays: it is a whole frame's; under another gate reference the state MEANS another frame), the map's generation.  Applied by settings_commit and, the group's
// half, by group_set: nowhere else.
struct SettingEnds { bool kept, gate, map_gen; };
constexpr SettingEnds SETTING_ENDS[N_SETTINGS] = {{true, true, true}, {true, true, false}, {true, false, true}, {true, false, true},
                                                  {false, false, false}, {false, false, false}, {true, true, false},
                                                  {false, true, false}};

// ---- a setter's proposal (the matcher's and the group's): `s` in force with its arguments applied, their range checked (INVALID_ARG)
inline FrameSettings propose_working_size(FrameSettings s, int max_w, int max_h) {
    if (max_w < 0 || max_h < 0 || (max_w == 0) != (max_h == 0))
        fail(SLIDEO_ERR_INVALID_ARG, "working size %dx%d: both sides positive, or 0, 0 for none", max_w, max_h);
    s.work_w = max_w; s.work_h = max_h;
    return s;
}
inline void frame_region_check(int src_w, int src_h, const double* M, int out_w, int out_h) {
    if (out_w < 1 || out_h < 1 || out_w > MAX_DIM || out_h > MAX_DIM)
        fail(SLIDEO_ERR_INVALID_ARG, "frame region: output size %dx%d outside 1..%d", out_w, out_h, MAX_DIM);
    if (src_w < 1 || src_h < 1 || src_w > MAX_DIM || src_h > MAX_DIM)
        fail(SLIDEO_ERR_INVALID_ARG, "frame region: source size %dx%d outside 1..%d", src_w, src_h, MAX_DIM);
    for (int i = 0; i < 9; ++i) if (!std::isfinite(M[i])) fail(SLIDEO_ERR_INVALID_ARG, "frame region: M[%d] is not finite", i);
    // W = M6 x + M7 y + M8 is affine over the destination rectangle: one sign at its four corners is one sign everywhere
    const double xs[2] = {0.0, (double)(out_w - 1)}, ys[2] = {0.0, (double)(out_h - 1)};
    int pos = 0, neg = 0;
    for (double y : ys) for (double x : xs) { const double W = M[6] * x + M[7] * y + M[8]; pos += W > 0.0; neg += W < 0.0; }
    if (pos != 4 && neg != 4)
        fail(SLIDEO_ERR_INVALID_ARG, "frame region: W = M6 x + M7 y + M8 is zero or changes sign over the corners of the %dx%d destination", out_w, out_h);
}
// M null: no region.  (The rectify_kernel instance — kind, tx, ty — is chosen at the commit.)
inline FrameSettings propose_frame_region(FrameSettings s, int src_w, int src_h, const double* M, int out_w, int out_h) {
    s.region = FrameRegion{};
    if (!M) return s;
    frame_region_check(src_w, src_h, M, out_w, out_h);
    s.region.set = true; s.region.src_w = src_w; s.region.src_h = src_h; s.region.out_w = out_w; s.region.out_h = out_h;
    for (int i = 0; i < 9; ++i) s.region.M[i] = M[i];
    return s;
}
// The lens commits under SET_FRAME_REGION like the region: it ends the kept frames, the gate state and the match sessions.  k1 == 0 and
// k2 == 0: off, and the other arguments are not looked at.  (The reach rule needs the region in force: frame_settings_rules.)
inline FrameSettings propose_frame_lens(FrameSettings s, int src_w, int src_h, double cx, double cy, double f, double k1, double k2) {
    s.lens = FrameLens{};
    if (k1 == 0.0 && k2 == 0.0) return s;
    if (src_w < 1 || src_h < 1 || src_w > MAX_DIM || src_h > MAX_DIM)
        fail(SLIDEO_ERR_INVALID_ARG, "frame lens: source size %dx%d outside 1..%d", src_w, src_h, MAX_DIM);
    const double a[5] = {cx, cy, f, k1, k2};
    static const char* const names[5] = {"cx", "cy", "f", "k1", "k2"};
    for (int i = 0; i < 5; ++i) if (!std::isfinite(a[i])) fail(SLIDEO_ERR_INVALID_ARG, "frame lens: %s is not finite", names[i]);
    if (!(f > 0.0)) fail(SLIDEO_ERR_INVALID_ARG, "frame lens: f %g: the normaliser is positive", f);
    const double q = 1.0 / (f * f);
    if (!std::isfinite(q) || !(q > 0.0)) fail(SLIDEO_ERR_INVALID_ARG, "frame lens: f %g: 1 / f^2 is not a positive finite number", f);
    s.lens.set = true; s.lens.src_w = src_w; s.lens.src_h = src_h;
    s.lens.cx = cx; s.lens.cy = cy; s.lens.f = f; s.lens.k1 = k1; s.lens.k2 = k2; s.lens.q = q;
    return s;
}
// The monotonicity rule of "Frame lens": d/dr (r g(r)) = 1 + 3 k1 s + 5 k2 s^2 > 0 (s = r2) at 0, at R2 and at the vertex
// -3 k1 / (10 k2) where that lies inside (0, R2): the radial map is strictly increasing over [0, sqrt(R2)]
inline bool frame_lens_monotone(double k1, double k2, double R2) {
    if (!std::isfinite(R2) || R2 < 0.0) return false;
    const auto d = [&](double s) { return 1.0 + 3.0 * k1 * s + 5.0 * k2 * s * s; };
    if (!(d(0.0) > 0.0) || !(d(R2) > 0.0)) return false;
    if (k2 != 0.0) {
        const double sv = -3.0 * k1 / (10.0 * k2);
        if (sv > 0.0 && sv < R2 && !(d(sv) > 0.0)) return false;
    }
    return true;
}
// The reach R2 of a lens beside a region (or none): the largest r2 of the ideal images of the destination's four corners (the image
// of the rectangle is convex, so a corner is its farthest point).  Not finite: W == 0 at a corner
inline double frame_lens_reach(const FrameLens& L, const FrameRegion& R) {
    const int dw = R.set ? R.out_w : L.src_w, dh = R.set ? R.out_h : L.src_h;
    const double xs[2] = {0.0, (double)(dw - 1)}, ys[2] = {0.0, (double)(dh - 1)};
    double R2 = 0.0;
    for (double y : ys) for (double x : xs) {
        double u = x, v = y;
        if (R.set) {
            const double* M = R.M;
            const double W = M[6] * x + M[7] * y + M[8];
            u = (M[0] * x + M[1] * y + M[2]) / W; v = (M[3] * x + M[4] * y + M[5]) / W;
        }
        const double r2 = ((u - L.cx) * (u - L.cx) + (v - L.cy) * (v - L.cy)) * L.q;
        if (!std::isfinite(r2)) return r2;              // (the rule then fails)
        if (r2 > R2) R2 = r2;
    }
    return R2;
}
// set false: no mask.  (The pyramid and the validity map are built at the commit.)
inline FrameSettings propose_frame_mask(FrameSettings s, bool set, int width, int height, int stride_bytes) {
    if (set && (width < 1 || height < 1 || stride_bytes < width))
        fail(SLIDEO_ERR_INVALID_ARG, "bad mask geometry w=%d h=%d stride=%d", width, height, stride_bytes);
    s.mask = set ? FrameMask{true, width, height} : FrameMask{};
    return s;
}
inline FrameSettings propose_frame_mask_scope(FrameSettings s, uint32_t scope) {
    if (scope == 0 || (scope & ~(uint32_t)(SLIDEO_MASK_DETECT | SLIDEO_MASK_GATE)))
        fail(SLIDEO_ERR_INVALID_ARG, "frame mask scope %u: a non-empty combination of SLIDEO_MASK_DETECT (1) and SLIDEO_MASK_GATE (2)", scope);
    s.mask_scope = scope;
    return s;
}
inline FrameSettings propose_direct_similarity(FrameSettings s, float t) {
    if (!(t >= 0.f) || t > 1.f) fail(SLIDEO_ERR_INVALID_ARG, "direct similarity %g: 0 (off) or 0 < t <= 1", (double)t);
    s.direct_t = t;
    return s;
}
inline FrameSettings propose_direct_scope(FrameSettings s, uint32_t scope) {
    if (scope != SLIDEO_DIRECT_WHOLE && scope != SLIDEO_DIRECT_VALID)
        fail(SLIDEO_ERR_INVALID_ARG, "direct scope %u: SLIDEO_DIRECT_WHOLE (0) or SLIDEO_DIRECT_VALID (1)", scope);
    s.direct_scope = scope;
    return s;
}

inline FrameSettings propose_yuv_description(FrameSettings s, int matrix, int range, int depth) {
    if (matrix != SLIDEO_YUV_MATRIX_BT601 && matrix != SLIDEO_YUV_MATRIX_BT709)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv description: matrix %d is neither SLIDEO_YUV_MATRIX_BT601 (0) nor SLIDEO_YUV_MATRIX_BT709 (1)", matrix);
    if (range != SLIDEO_YUV_RANGE_LIMITED && range != SLIDEO_YUV_RANGE_FULL)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv description: range %d is neither SLIDEO_YUV_RANGE_LIMITED (0) nor SLIDEO_YUV_RANGE_FULL (1)", range);
    if (depth != SLIDEO_YUV_DEPTH_8 && depth != SLIDEO_YUV_DEPTH_10_MSB && depth != SLIDEO_YUV_DEPTH_10_LSB)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv description: depth %d is none of SLIDEO_YUV_DEPTH_8 (0), _10_MSB (1), _10_LSB (2)", depth);
    s.yuv.matrix = matrix; s.yuv.range = range; s.yuv.depth = depth;       // (the sampling and the chroma filter stay: each is set on its own)
    return s;
}
// The sampling commits under SET_YUV_DESCRIPTION like the description: it ends the kept frames and resets the gate
inline FrameSettings propose_yuv_sampling(FrameSettings s, int sampling) {
    if (sampling != SLIDEO_YUV_SAMPLING_420 && sampling != SLIDEO_YUV_SAMPLING_422 && sampling != SLIDEO_YUV_SAMPLING_444 &&
        sampling != SLIDEO_YUV_SAMPLING_422_PACKED)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv sampling: %d is none of SLIDEO_YUV_SAMPLING_420 (0), _422 (1), _444 (2), _422_PACKED (3)", sampling);
    s.yuv.sampling = sampling;
    return s;
}
// The chroma filter commits under SET_YUV_DESCRIPTION like the sampling: it ends the kept frames and resets the gate
inline FrameSettings propose_yuv_chroma(FrameSettings s, int filter) {
    if (filter != SLIDEO_YUV_CHROMA_NEAREST && filter != SLIDEO_YUV_CHROMA_BILINEAR_LEFT && filter != SLIDEO_YUV_CHROMA_BILINEAR_CENTER &&
        filter != SLIDEO_YUV_CHROMA_BILINEAR_TOPLEFT)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv chroma filter: %d is none of SLIDEO_YUV_CHROMA_NEAREST (0), _BILINEAR_LEFT (1), _BILINEAR_CENTER (2), "
             "_BILINEAR_TOPLEFT (3)", filter);
    s.yuv.chroma = filter;
    return s;
}
// The transfer commits under SET_YUV_DESCRIPTION like the sampling: it ends the kept frames and resets the gate
inline FrameSettings propose_yuv_transfer(FrameSettings s, int transfer, float white_nits) {
    if (transfer != SLIDEO_YUV_TRANSFER_SDR && transfer != SLIDEO_YUV_TRANSFER_HLG && transfer != SLIDEO_YUV_TRANSFER_PQ)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv transfer: %d is none of SLIDEO_YUV_TRANSFER_SDR (0), _HLG (1), _PQ (2)", transfer);
    if (transfer == SLIDEO_YUV_TRANSFER_SDR) {
        if (!(white_nits == 0.f)) fail(SLIDEO_ERR_INVALID_ARG, "yuv transfer: white_nits %g under SLIDEO_YUV_TRANSFER_SDR must be 0", (double)white_nits);
    } else if (!(white_nits == 0.f) && !(std::isfinite(white_nits) && white_nits >= 1.f && white_nits <= 10000.f))
        fail(SLIDEO_ERR_INVALID_ARG, "yuv transfer: white_nits %g: 0 (203, the BT.2408 reference white) or a finite value in 1 .. 10000", (double)white_nits);
    s.yuv.transfer = transfer;
    s.yuv.white_nits = transfer == SLIDEO_YUV_TRANSFER_SDR ? 0.f : white_nits == 0.f ? 203.f : white_nits;
    return s;
}
// The weight rule of "YUV chroma filter": out12 = wh[2][3], wv[2][3], [parity][sample k - 1, k, k + 1], in quarters.  An axis that
// is not interpolated — both under NEAREST and 4:4:4, the vertical one under the 4:2:2 forms — is (0, 4, 0) twice; a co-sited axis is
// (0, 4, 0), (0, 2, 2); a centred one (1, 3, 0), (0, 3, 1).  false: not a filter or not a sampling
inline bool yuv_chroma_weights(int filter, int sampling, int32_t* out12) {
    if (filter < SLIDEO_YUV_CHROMA_NEAREST || filter > SLIDEO_YUV_CHROMA_BILINEAR_TOPLEFT) return false;
    if (sampling < SLIDEO_YUV_SAMPLING_420 || sampling > SLIDEO_YUV_SAMPLING_422_PACKED) return false;
    static const int32_t NONE[6] = {0, 4, 0, 0, 4, 0}, COSITED[6] = {0, 4, 0, 0, 2, 2}, CENTRED[6] = {1, 3, 0, 0, 3, 1};
    const bool on = filter != SLIDEO_YUV_CHROMA_NEAREST && sampling != SLIDEO_YUV_SAMPLING_444;
    const int32_t* wh = !on ? NONE : filter == SLIDEO_YUV_CHROMA_BILINEAR_CENTER ? CENTRED : COSITED;
    const int32_t* wv = !on || sampling != SLIDEO_YUV_SAMPLING_420 ? NONE : filter == SLIDEO_YUV_CHROMA_BILINEAR_TOPLEFT ? COSITED : CENTRED;
    for (int i = 0; i < 6; ++i) { out12[i] = wh[i]; out12[6 + i] = wv[i]; }
    return true;
}

// ---- the frame pixel format (include/slideo_amd.h "Frame pixel format") -----------------------------------------------------------
// bytes per pixel of a row (3 or 4; 1: a plane's) and planes (1 or 3) of a format; false: not a format
inline bool pixel_format_info(int format, int* bytes_per_pixel, int* planes) {
    if (format < SLIDEO_PIXEL_BGR8 || format > SLIDEO_PIXEL_PLANAR_GBR8) return false;
    const bool planar = format >= SLIDEO_PIXEL_PLANAR_RGB8, four = format >= SLIDEO_PIXEL_BGRA8 && !planar;
    if (bytes_per_pixel) *bytes_per_pixel = planar ? 1 : four ? 4 : 3;
    if (planes) *planes = planar ? 3 : 1;
    return true;
}
inline const char* pixel_format_name(int format) {
    static const char* const names[] = {"SLIDEO_PIXEL_BGR8", "SLIDEO_PIXEL_RGB8", "SLIDEO_PIXEL_BGRA8", "SLIDEO_PIXEL_RGBA8", "SLIDEO_PIXEL_ARGB8",
                                        "SLIDEO_PIXEL_ABGR8", "SLIDEO_PIXEL_PLANAR_RGB8", "SLIDEO_PIXEL_PLANAR_BGR8", "SLIDEO_PIXEL_PLANAR_GBR8"};
    return format >= SLIDEO_PIXEL_BGR8 && format <= SLIDEO_PIXEL_PLANAR_GBR8 ? names[format] : "?";
}
// where a pixel's B, G and R lie: the byte of a packed pixel, the plane of a planar frame
inline void pixel_format_channels(int format, int* b, int* g, int* r) {
    static const int pos[9][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {3, 2, 1}, {1, 2, 3}, {2, 1, 0}, {0, 1, 2}, {1, 0, 2}};
    *b = pos[format][0]; *g = pos[format][1]; *r = pos[format][2];
}
// The format commits under SET_YUV_DESCRIPTION like the sampling: it ends the kept frames and resets the gate
inline FrameSettings propose_pixel_format(FrameSettings s, int format) {
    if (!pixel_format_info(format, nullptr, nullptr))
        fail(SLIDEO_ERR_INVALID_ARG, "pixel format: %d is none of SLIDEO_PIXEL_BGR8 (0) .. SLIDEO_PIXEL_PLANAR_GBR8 (8)", format);
    s.pixel_format = format;
    return s;
}
// The layout rules of a frame under a format other than SLIDEO_PIXEL_BGR8 (whose rules and messages are validate_image's); returns the
// bytes of one frame.  frame_stride < 0: a single frame, no stride to check.
inline int64_t pixel_format_validate(int format, int w, int h, int stride, int64_t frame_stride) {
    int bpp = 0, planes = 0;
    if (!pixel_format_info(format, &bpp, &planes)) fail(SLIDEO_ERR_INVALID_ARG, "pixel format: %d is not a format", format);
    const char* name = pixel_format_name(format);
    if (w < 1 || h < 1) fail(SLIDEO_ERR_INVALID_ARG, "bad image geometry w=%d h=%d stride=%d", w, h, stride);
    if ((int64_t)stride < (int64_t)bpp * w) {
        if (planes == 3) fail(SLIDEO_ERR_INVALID_ARG, "%s: stride_bytes %d < width %d (the row stride of every plane)", name, stride, w);
        fail(SLIDEO_ERR_INVALID_ARG, "%s: stride_bytes %d < %d * width %d", name, stride, bpp, w);
    }
    const int64_t span = (int64_t)planes * h * stride;
    if (frame_stride >= 0 && frame_stride < span) {
        if (planes == 3)
            fail(SLIDEO_ERR_INVALID_ARG, "%s: frame_stride %lld does not cover the frame's three planes (3 * height %d * stride_bytes %d = %lld)", name,
                 (long long)frame_stride, h, stride, (long long)span);
        fail(SLIDEO_ERR_INVALID_ARG, "%s: frame_stride %lld smaller than one frame (height %d * stride_bytes %d = %lld)", name, (long long)frame_stride, h,
             stride, (long long)span);
    }
    return span;
}

// ---- the frame levels (include/slideo_amd.h "Frame levels") ---------------------------------------------------------------------------
inline bool frame_levels_identity(const uint8_t* lut768) {
    for (int i = 0; i < 768; ++i) if (lut768[i] != (uint8_t)(i & 255)) return false;
    return true;
}
// The table commits under SET_YUV_DESCRIPTION like the pixel format: it ends the kept frames and resets the gate.  lut768 null, or
// the identity: off.  session_open: the matcher's levels histogram is open (a table learnt on levelled frames is not the source's)
inline FrameSettings propose_frame_levels(FrameSettings s, const uint8_t* lut768, bool session_open) {
    if (session_open)
        fail(SLIDEO_ERR_STATE, "frame levels: the levels histogram is open, and a table learnt on levelled frames is not the source's "
                               "(slideo_matcher_levels_end first)");
    s.levels = FrameLevels{};
    if (!lut768 || frame_levels_identity(lut768)) return s;
    s.levels.set = true;
    for (int i = 0; i < 768; ++i) s.levels.lut[i] = lut768[i];
    return s;
}
// The stretch table of the points (lo, hi) per channel: lut[c][x] = clamp(floor((510 (x - lo) + (hi - lo)) / (2 (hi - lo))), 0, 255),
// the rounded 255 (x - lo) / (hi - lo) in integers; (0, 255) is the identity
inline void frame_levels_lut(const int32_t* lo, const int32_t* hi, uint8_t* lut768) {
    static const char* const names[3] = {"B", "G", "R"};
    for (int c = 0; c < 3; ++c)
        if (lo[c] < 0 || hi[c] > 255 || lo[c] >= hi[c])
            fail(SLIDEO_ERR_INVALID_ARG, "frame levels: channel %d (%s) has lo %d, hi %d: 0 <= lo < hi <= 255", c, names[c], lo[c], hi[c]);
    for (int c = 0; c < 3; ++c) {
        const int d = hi[c] - lo[c];
        for (int x = 0; x < 256; ++x) {
            const int num = 510 * (x - lo[c]) + d;             // (floor of a negative quotient: below 0 either way)
            const int v = num < 0 ? 0 : num / (2 * d);
            lut768[c * 256 + x] = (uint8_t)(v > 255 ? 255 : v);
        }
    }
}
// The points of a histogram hist[c * 256 + v] at (low_ppm, high_ppm): per channel, with total its samples, lo is the value of the
// sample of ascending rank floor(total * low_ppm / 1e6) (0-based) and hi that of rank total - 1 - floor(total * high_ppm / 1e6);
// reported as they are (frame_levels_lut is what refuses hi <= lo).  A channel without samples: STATE
constexpr int LEVELS_MAX_PPM = 1000000;
inline uint64_t levels_ppm_rank(uint64_t total, uint64_t ppm) {           // floor(total * ppm / 1e6) without a 128-bit product
    return total / 1000000u * ppm + total % 1000000u * ppm / 1000000u;
}
inline int levels_value_at(const uint64_t* hist256, uint64_t rank) {      // the value of the sample of ascending rank `rank` < total
    uint64_t below = 0;
    for (int v = 0; v < 256; ++v) { below += hist256[v]; if (rank < below) return v; }
    return 255;
}
inline void levels_points(const uint64_t* hist768, int low_ppm, int high_ppm, int32_t* lo, int32_t* hi) {
    if (low_ppm < 0 || low_ppm > LEVELS_MAX_PPM || high_ppm < 0 || high_ppm > LEVELS_MAX_PPM)
        fail(SLIDEO_ERR_INVALID_ARG, "levels_points: low_ppm %d, high_ppm %d outside 0..%d", low_ppm, high_ppm, LEVELS_MAX_PPM);
    for (int c = 0; c < 3; ++c) {
        const uint64_t* h = hist768 + c * 256;
        uint64_t total = 0;
        for (int v = 0; v < 256; ++v) total += h[v];
        if (total == 0) fail(SLIDEO_ERR_STATE, "the levels histogram has observed no frame");
        const uint64_t rl = std::min(levels_ppm_rank(total, (uint64_t)low_ppm), total - 1);
        const uint64_t cut = std::min(levels_ppm_rank(total, (uint64_t)high_ppm), total - 1);
        lo[c] = levels_value_at(h, rl);
        hi[c] = levels_value_at(h, total - 1 - cut);
    }
}

// ---- the frame shading (include/slideo_amd.h "Frame shading") -------------------------------------------------------------------------
inline bool shading_cell_ok(int cell) { return cell == 16 || cell == 32 || cell == 64; }
// The field commits under SET_YUV_DESCRIPTION like the levels table: it ends the kept frames and resets the gate.  gains null, or
// every node 256: off (aw, ah and cell are then not looked at).  A gain of 0 is refused by its node
inline FrameSettings propose_frame_shading(FrameSettings s, int aw, int ah, int cell, const uint16_t* gains) {
    s.shading = FrameShading{};
    if (!gains) return s;
    if (!shading_cell_ok(cell)) fail(SLIDEO_ERR_INVALID_ARG, "frame shading: cell %d is none of 16, 32, 64", cell);
    if (aw < 1 || ah < 1 || aw > MAX_DIM || ah > MAX_DIM) fail(SLIDEO_ERR_INVALID_ARG, "frame shading: analysed size %dx%d outside 1..%d", aw, ah, MAX_DIM);
    const int gw = (aw + cell - 1) / cell, gh = (ah + cell - 1) / cell;
    const size_t nodes = (size_t)(gw + 1) * (gh + 1);
    bool identity = true;
    for (size_t k = 0; k < nodes; ++k) {
        if (gains[k] == 0)
            fail(SLIDEO_ERR_INVALID_ARG, "frame shading: node (%d, %d) has gain 0: every gain is at least 1 (Q8.8, 256 = 1.0)", (int)(k % (size_t)(gw + 1)),
                 (int)(k / (size_t)(gw + 1)));
        identity &= gains[k] == 256;
    }
    if (identity) return s;
    s.shading.set = true; s.shading.aw = aw; s.shading.ah = ah; s.shading.cell = cell;
    s.shading.gains = std::make_shared<const std::vector<uint16_t>>(gains, gains + nodes);
    return s;
}
// The rule of the header for one pixel of a B, G or R byte `in` at (x, y): the definition the kernel and the restatement are held to
inline uint8_t frame_shading_pixel(const uint16_t* g, int gw, int cell, int x, int y, uint8_t in) {
    const int sh = cell == 16 ? 4 : cell == 32 ? 5 : 6, i = x >> sh, j = y >> sh, fx = x - (i << sh), fy = y - (j << sh), p = gw + 1;
    const uint32_t L = (uint32_t)g[j * p + i] * (uint32_t)(cell - fy) + (uint32_t)g[(j + 1) * p + i] * (uint32_t)fy;
    const uint32_t R = (uint32_t)g[j * p + i + 1] * (uint32_t)(cell - fy) + (uint32_t)g[(j + 1) * p + i + 1] * (uint32_t)fy;
    const uint32_t G = (L * (uint32_t)(cell - fx) + R * (uint32_t)fx + (uint32_t)(cell * cell / 2)) >> (2 * sh);
    const uint32_t v = ((uint32_t)in * G + 128u) >> 8;
    return (uint8_t)(v < 255u ? v : 255u);
}

inline FrameSettings propose_gate_reference(FrameSettings s, uint32_t ref) {
    if (ref != SLIDEO_GATE_PREVIOUS && ref != SLIDEO_GATE_ANCHOR)
        fail(SLIDEO_ERR_INVALID_ARG, "gate reference %u: SLIDEO_GATE_PREVIOUS (0) or SLIDEO_GATE_ANCHOR (1)", ref);
    s.gate_ref = ref;
    return s;
}
// The gate settle commits under SET_GATE_REFERENCE: the state means something else, so the gate resets (its SETTING_ENDS row)
inline FrameSettings propose_gate_settle(FrameSettings s, float settle_similarity, int32_t max_defer) {
    if (!(settle_similarity >= 0.f) || settle_similarity > 1.f)
        fail(SLIDEO_ERR_INVALID_ARG, "gate settle: settle_similarity %g: 0 (off) or 0 < s <= 1", (double)settle_similarity);
    if (max_defer < 0) fail(SLIDEO_ERR_INVALID_ARG, "gate settle: max_defer %d: 0 <= max_defer <= INT32_MAX", max_defer);
    s.settle_similarity = settle_similarity; s.settle_max_defer = max_defer;
    return s;
}
// The gate memory commits under SET_GATE_REFERENCE as the settle does: the state means something else, so the gate resets
inline FrameSettings propose_gate_memory(FrameSettings s, int32_t capacity) {
    if (capacity < 0 || capacity > SLIDEO_GATE_MEMORY_MAX)
        fail(SLIDEO_ERR_INVALID_ARG, "gate memory: capacity %d: 0 (off) or 1 .. %d", capacity, SLIDEO_GATE_MEMORY_MAX);
    s.gate_memory = capacity;
    return s;
}
// The group's rule for a gate memory (include/slideo_amd.h "Gate memory"): the chain's baton carries three buffers, not a ring, and
// a one-frame halo carries no memory, so a memory that is on needs a group of one member.  Setting it off always passes.
inline void gate_memory_group_rule(int members, int32_t capacity) {
    if (capacity > 0 && members > 1)
        fail(SLIDEO_ERR_UNSUPPORTED, "a gate memory in a group of %d members: the gate state a shard hands on carries no memory (a group of "
             "one member, or a single matcher)", members);
}
// The gate state as a record holds no memory (record version 1): refused by name while a memory is on
inline void gate_record_memory_rule(int32_t gate_memory) {
    if (gate_memory > 0)
        fail(SLIDEO_ERR_UNSUPPORTED, "the gate state record (version %u) does not carry the gate memory: not while a gate memory of %d is on "
             "(slideo_matcher_set_gate_memory(m, 0) first)", 1u, gate_memory);
}
// The group's rule for a gate settle (include/slideo_amd.h "Gate settle"): it needs ANCHOR, which needs a group of one member
// or the group gate order CHAIN ("Group gate order").  Setting it off always passes.
inline void gate_settle_group_rule(int members, float settle_similarity, uint32_t order = SLIDEO_GROUP_GATE_HALO) {
    if (settle_similarity > 0.f && members > 1 && order != SLIDEO_GROUP_GATE_CHAIN)
        fail(SLIDEO_ERR_UNSUPPORTED, "a gate settle in a group of %d members: it runs under SLIDEO_GATE_ANCHOR, which a group of more than "
             "one member does not support (a group of one member, or a single matcher)", members);
}
// The group's rule for a gate reference (include/slideo_amd.h "Gate reference"): a shard's anchor depends on every flag before the
// shard, which the one-frame halo that primes a shard cannot supply, so ANCHOR needs a group of one member — or the group gate order
// CHAIN, under which a shard receives its predecessor's whole state ("Group gate order").  PREVIOUS always passes.
inline void gate_reference_group_rule(int members, uint32_t ref, uint32_t order = SLIDEO_GROUP_GATE_HALO) {
    if (ref == SLIDEO_GATE_ANCHOR && members > 1 && order != SLIDEO_GROUP_GATE_CHAIN)
        fail(SLIDEO_ERR_UNSUPPORTED, "gate reference SLIDEO_GATE_ANCHOR in a group of %d members: a shard's anchor depends on every flag before "
             "the shard, and the one frame that primes a shard cannot supply it (a group of one member, or a single matcher)", members);
}
// The group gate order's proposal and its rule (include/slideo_amd.h "Group gate order"): HALO primes a shard from one frame, which
// carries neither an anchor nor a settle's state, so with more than one member it stands beside PREVIOUS without a settle only.  The
// third of the three set calls that can complete the refused combination.
inline uint32_t propose_group_gate_order(uint32_t order) {
    if (order != SLIDEO_GROUP_GATE_HALO && order != SLIDEO_GROUP_GATE_CHAIN)
        fail(SLIDEO_ERR_INVALID_ARG, "group gate order %u: SLIDEO_GROUP_GATE_HALO (0) or SLIDEO_GROUP_GATE_CHAIN (1)", order);
    return order;
}
inline void group_gate_order_rule(int members, uint32_t order, uint32_t gate_ref, float settle_similarity) {
    if (order == SLIDEO_GROUP_GATE_CHAIN || members <= 1) return;
    if (gate_ref == SLIDEO_GATE_ANCHOR || settle_similarity > 0.f)
        fail(SLIDEO_ERR_UNSUPPORTED, "group gate order SLIDEO_GROUP_GATE_HALO in a group of %d members under %s: the one frame that primes a shard "
             "carries neither an anchor nor a settle's state (slideo_group_set_gate_settle(g, 0, 0) and "
             "slideo_group_set_gate_reference(g, SLIDEO_GATE_PREVIOUS) before going back)", members,
             settle_similarity > 0.f ? "a gate settle" : "SLIDEO_GATE_ANCHOR");
}

// ---- the gate state as a record (include/slideo_amd.h "Gate state record") ---------------------------------------------------------
// A fixed little-endian header of GATE_RECORD_HEADER bytes — magic, version, has, gate reference, settle on, sw, sh, d: eight 32-bit
// words — then, has: the anchor's small image (under PREVIOUS: the last small image) and, under a settle, the previous frame's, 3 *
// sw * sh bytes each.  "none": the header alone, sw = sh = d = 0.
constexpr uint32_t GATE_RECORD_MAGIC = 0x54534753u;      // "SGST"
constexpr uint32_t GATE_RECORD_VERSION = 1;
constexpr int64_t GATE_RECORD_HEADER = 32;
struct GateRecordHead {
    bool has = false;
    uint32_t gate_ref = SLIDEO_GATE_PREVIOUS;
    bool settle = false;
    int32_t sw = 0, sh = 0;
    uint32_t d = 0;
    int64_t image_bytes() const { return has ? (int64_t)sw * sh * 3 : 0; }
    int64_t bytes() const { return GATE_RECORD_HEADER + image_bytes() * (settle ? 2 : 1); }
};
inline void gate_record_put32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
inline uint32_t gate_record_get32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void gate_record_encode(const GateRecordHead& h, uint8_t* out32) {
    const uint32_t w[8] = {GATE_RECORD_MAGIC, GATE_RECORD_VERSION, h.has ? 1u : 0u, h.gate_ref, h.settle ? 1u : 0u, (uint32_t)h.sw, (uint32_t)h.sh, h.d};
    for (int i = 0; i < 8; ++i) gate_record_put32(out32 + 4 * i, w[i]);
}
// The header of a record of `bytes` bytes for a matcher under (gate_ref, settle_similarity, max_defer, small_area): every refusal is
// SLIDEO_ERR_INVALID_ARG with the rule named; nothing is written anywhere.
inline GateRecordHead gate_record_validate(const uint8_t* rec, int64_t bytes, uint32_t gate_ref, float settle_similarity, int32_t max_defer,
                                           int small_area) {
    if (!rec) fail(SLIDEO_ERR_INVALID_ARG, "gate state record: null record");
    if (bytes < GATE_RECORD_HEADER)
        fail(SLIDEO_ERR_INVALID_ARG, "gate state record: %lld bytes, the header alone takes %lld", (long long)bytes, (long long)GATE_RECORD_HEADER);
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) w[i] = gate_record_get32(rec + 4 * i);
    if (w[0] != GATE_RECORD_MAGIC) fail(SLIDEO_ERR_INVALID_ARG, "gate state record: magic %08x is not %08x", w[0], GATE_RECORD_MAGIC);
    if (w[1] != GATE_RECORD_VERSION) fail(SLIDEO_ERR_INVALID_ARG, "gate state record: version %u, this library reads version %u", w[1], GATE_RECORD_VERSION);
    if (w[2] > 1 || w[4] > 1) fail(SLIDEO_ERR_INVALID_ARG, "gate state record: has %u and settle %u must be 0 or 1", w[2], w[4]);
    GateRecordHead h;
    h.has = w[2] == 1; h.gate_ref = w[3]; h.settle = w[4] == 1; h.sw = (int32_t)w[5]; h.sh = (int32_t)w[6]; h.d = w[7];
    const bool settle = settle_similarity > 0.f;
    if (h.gate_ref != gate_ref)
        fail(SLIDEO_ERR_INVALID_ARG, "gate state record: made under gate reference %u, the matcher's is %u", h.gate_ref, gate_ref);
    if (h.settle != settle)
        fail(SLIDEO_ERR_INVALID_ARG, "gate state record: made with the gate settle %s, the matcher's is %s", h.settle ? "on" : "off", settle ? "on" : "off");
    if (!h.has) {
        if (h.sw != 0 || h.sh != 0 || h.d != 0) fail(SLIDEO_ERR_INVALID_ARG, "gate state record: a record of \"none\" with sw %d, sh %d, d %u", h.sw, h.sh, h.d);
    } else {
        // (slideo_matcher_gate_reset's size check)
        if (h.sw < 1 || h.sh < 1 || (int64_t)h.sw * h.sh > small_area)
            fail(SLIDEO_ERR_INVALID_ARG, "gate state record: a %dx%d small image (at most small_area = %d pixels)", h.sw, h.sh, small_area);
        if (h.d > (settle ? (uint32_t)max_defer : 0u))
            fail(SLIDEO_ERR_INVALID_ARG, "gate state record: deferral count %u beyond the matcher's max_defer %d", h.d, settle ? max_defer : 0);
    }
    if (bytes != h.bytes()) fail(SLIDEO_ERR_INVALID_ARG, "gate state record: %lld bytes, its header describes %lld", (long long)bytes, (long long)h.bytes());
    return h;
}
// frames per gated unit under SLIDEO_GATE_ANCHOR: the unit's table of dot products takes 8 n^2 bytes
constexpr int GATE_ANCHOR_MAX_UNIT = 1024;

// The seven integers of the fixed-point conversion under (matrix, range) — CY, CUB, CUG, CVG, CVR, y_offset, SHIFT —, arguments
// checked by the caller.  (BT601, LIMITED): cvtColor's literals.  Every other pair by the rule of include/slideo_amd.h, in float64.
inline void yuv_coefficients(int matrix, int range, int32_t* out7) {
    out7[6] = 20;
    if (matrix == SLIDEO_YUV_MATRIX_BT601 && range == SLIDEO_YUV_RANGE_LIMITED) {
        out7[0] = 1220542; out7[1] = 2116026; out7[2] = -409993; out7[3] = -852492; out7[4] = 1673527; out7[5] = 16;
        return;
    }
    const bool bt709 = matrix == SLIDEO_YUV_MATRIX_BT709, full = range == SLIDEO_YUV_RANGE_FULL;
    const double Kr = bt709 ? 0.2126 : 0.299, Kb = bt709 ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
    const double sy = full ? 1.0 : 255.0 / 219.0, sc = full ? 1.0 : 255.0 / 224.0, one = 1048576.0;
    out7[0] = (int32_t)std::rint(sy * one);
    out7[1] = (int32_t)std::rint(sc * 2.0 * (1.0 - Kb) * one);
    out7[2] = -(int32_t)std::rint(sc * 2.0 * (1.0 - Kb) * Kb / Kg * one);
    out7[3] = -(int32_t)std::rint(sc * 2.0 * (1.0 - Kr) * Kr / Kg * one);
    out7[4] = (int32_t)std::rint(sc * 2.0 * (1.0 - Kr) * one);
    out7[5] = full ? 0 : 16;
}

// ---- the integers of "YUV transfer" (include/slideo_amd.h), in float64 ------------------------------------------------------------
constexpr int YUV_TR_SHIFT = 18, YUV_TR_LIN = 1024, YUV_TR_OUT = 4096, YUV_TR_WHITE = 16383, YUV_TR_GAMUT_SHIFT = 14;
// step 2: CY, CUB, CUG, CVG, CVR, y_offset, SHIFT of the BT.2020 non-constant-luminance matrix at 10 bits under `range`
inline void yuv_transfer_coefficients(int range, int32_t* out7) {
    const bool full = range == SLIDEO_YUV_RANGE_FULL;
    const double Kr = 0.2627, Kb = 0.0593, Kg = 1.0 - Kr - Kb;
    const double sy = full ? 1.0 : 1023.0 / 876.0, sc = full ? 1.0 : 1023.0 / 896.0, one = (double)(1 << YUV_TR_SHIFT);
    out7[0] = (int32_t)std::rint(sy * one);
    out7[1] = (int32_t)std::rint(sc * 2.0 * (1.0 - Kb) * one);
    out7[2] = -(int32_t)std::rint(sc * 2.0 * (1.0 - Kb) * Kb / Kg * one);
    out7[3] = -(int32_t)std::rint(sc * 2.0 * (1.0 - Kr) * Kr / Kg * one);
    out7[4] = (int32_t)std::rint(sc * 2.0 * (1.0 - Kr) * one);
    out7[5] = full ? 0 : 64;
    out7[6] = YUV_TR_SHIFT;
}
inline void mat3_inverse(const double* m, double* o) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double d = m[0] * c0 + m[1] * c1 + m[2] * c2;
    o[0] = c0 / d; o[1] = (m[2] * m[7] - m[1] * m[8]) / d; o[2] = (m[1] * m[5] - m[2] * m[4]) / d;
    o[3] = c1 / d; o[4] = (m[0] * m[8] - m[2] * m[6]) / d; o[5] = (m[2] * m[3] - m[0] * m[5]) / d;
    o[6] = c2 / d; o[7] = (m[1] * m[6] - m[0] * m[7]) / d; o[8] = (m[0] * m[4] - m[1] * m[3]) / d;
}
// RGB -> XYZ of a set of primaries (x, y of R, G, B) and the D65 white point: the columns are the primaries' XYZ, scaled so that
// RGB = (1, 1, 1) is the white
inline void yuv_transfer_rgb_to_xyz(const double* xy6, double* M9) {
    double P[9], W[3] = {0.3127 / 0.3290, 1.0, (1.0 - 0.3127 - 0.3290) / 0.3290};
    for (int c = 0; c < 3; ++c) { P[c] = xy6[2 * c] / xy6[2 * c + 1]; P[3 + c] = 1.0; P[6 + c] = (1.0 - xy6[2 * c] - xy6[2 * c + 1]) / xy6[2 * c + 1]; }
    double I[9];
    mat3_inverse(P, I);
    for (int c = 0; c < 3; ++c) {
        const double s = I[3 * c] * W[0] + I[3 * c + 1] * W[1] + I[3 * c + 2] * W[2];
        for (int r = 0; r < 3; ++r) M9[3 * r + c] = P[3 * r + c] * s;
    }
}
// step 4: BT.2020 -> BT.709 linear light, off the diagonal rint(G 2^14), the diagonal such that every row sums to 2^14
inline void yuv_transfer_gamut(int32_t* out9) {
    static const double P709[6] = {0.640, 0.330, 0.300, 0.600, 0.150, 0.060}, P2020[6] = {0.708, 0.292, 0.170, 0.797, 0.131, 0.046};
    double A[9], B[9], Ai[9];
    yuv_transfer_rgb_to_xyz(P709, A);
    yuv_transfer_rgb_to_xyz(P2020, B);
    mat3_inverse(A, Ai);
    for (int r = 0; r < 3; ++r) {
        int32_t off = 0;
        for (int c = 0; c < 3; ++c) {
            if (c == r) continue;
            const double g = Ai[3 * r] * B[c] + Ai[3 * r + 1] * B[3 + c] + Ai[3 * r + 2] * B[6 + c];
            out9[3 * r + c] = (int32_t)std::rint(g * (double)(1 << YUV_TR_GAMUT_SHIFT));
            off += out9[3 * r + c];
        }
        out9[3 * r + r] = (1 << YUV_TR_GAMUT_SHIFT) - off;
    }
}
// the display light in nits of the signal e in 0..1: ST 2084's EOTF; HLG's inverse OETF with the 1.2 system gamma of a nominal
// 1000-nit display, per channel
inline double yuv_transfer_nits(int transfer, double e) {
    if (transfer == SLIDEO_YUV_TRANSFER_PQ) {
        const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
        const double p = std::pow(e, 1.0 / m2);
        return 10000.0 * std::pow(std::max(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1);
    }
    const double a = 0.17883277, b = 0.28466892, c = 0.55991073;
    const double E = e <= 0.5 ? e * e / 3.0 : (std::exp((e - c) / a) + b) / 12.0;
    return 1000.0 * std::pow(E, 1.2);
}
// steps 3 and 5: LIN[i] = rint(16383 min(1, nits(i / 1023) / white_nits)), OUT[i] = rint(255 srgb_oetf(i / 4095)).  white_nits as
// resolved (never 0)
inline void yuv_transfer_lin_out(int transfer, double white_nits, uint16_t* lin1024, uint8_t* out4096) {
    for (int i = 0; i < YUV_TR_LIN; ++i)
        lin1024[i] = (uint16_t)std::rint((double)YUV_TR_WHITE * std::min(1.0, yuv_transfer_nits(transfer, (double)i / 1023.0) / white_nits));
    for (int i = 0; i < YUV_TR_OUT; ++i) {
        const double l = (double)i / 4095.0;
        out4096[i] = (uint8_t)std::rint(255.0 * (l <= 0.0031308 ? 12.92 * l : 1.055 * std::pow(l, 1.0 / 2.4) - 0.055));
    }
}
// slideo_yuv_transfer_tables: the whole definition; every output may be null.  false: not a transfer with tables (SDR has none), not
// a range, or nits outside the setter's rule
inline bool yuv_transfer_tables(int transfer, int range, float white_nits, int32_t* coef7, int32_t* gamut9, uint16_t* lin1024, uint8_t* out4096) {
    if (transfer != SLIDEO_YUV_TRANSFER_HLG && transfer != SLIDEO_YUV_TRANSFER_PQ) return false;
    if (range != SLIDEO_YUV_RANGE_LIMITED && range != SLIDEO_YUV_RANGE_FULL) return false;
    if (!(white_nits == 0.f) && !(std::isfinite(white_nits) && white_nits >= 1.f && white_nits <= 10000.f)) return false;
    if (coef7) yuv_transfer_coefficients(range, coef7);
    if (gamut9) yuv_transfer_gamut(gamut9);
    if (lin1024 || out4096) {
        uint16_t lin[YUV_TR_LIN];
        uint8_t out[YUV_TR_OUT];
        yuv_transfer_lin_out(transfer, white_nits == 0.f ? 203.0 : (double)white_nits, lin, out);
        if (lin1024) std::copy(lin, lin + YUV_TR_LIN, lin1024);
        if (out4096) std::copy(out, out + YUV_TR_OUT, out4096);
    }
    return true;
}

// The layout rules of include/slideo_amd.h "YUV 4:2:0 frames" for samples of `bps` bytes (1; 2: the 16-bit containers of "YUV
// colour description", whose rules count two bytes per sample); returns the bytes of one frame (its furthest byte + 1).
// frame_stride < 0: a single frame, no stride to check.  `sampling` other than 420: the rules of "YUV sampling"
// (yuv_sampled_validate); under 420 every rule and every message is as it was before the sampling existed.
inline int64_t yuv_sampled_validate(int w, int h, const slideo_yuv420_layout* L, int64_t frame_stride, int bps, int sampling);
inline int64_t yuv420_validate(int w, int h, const slideo_yuv420_layout* L, int64_t frame_stride, int bps, int sampling = SLIDEO_YUV_SAMPLING_420) {
    if (sampling != SLIDEO_YUV_SAMPLING_420) return yuv_sampled_validate(w, h, L, frame_stride, bps, sampling);
    if (w < 1 || h < 1) fail(SLIDEO_ERR_INVALID_ARG, "bad image geometry w=%d h=%d", w, h);
    if ((w | h) & 1) fail(SLIDEO_ERR_UNSUPPORTED, "yuv420: width and height must be even (%dx%d), as cvtColor requires", w, h);
    if (w > MAX_DIM || h > MAX_DIM) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", w, h, MAX_DIM);
    if (L->uv_step != 1 && L->uv_step != 2) fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: uv_step %d is neither 1 (planar) nor 2 (interleaved)", L->uv_step);
    if (L->u_offset < 0 || L->v_offset < 0) fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: negative plane offset");
    const int cw = w / 2, ch = h / 2;
    if (bps == 1) {
        if (L->y_stride < w) fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: y_stride %d < width %d", L->y_stride, w);
        if ((int64_t)L->uv_stride < (int64_t)cw * L->uv_step)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: uv_stride %d < %d (width/2 chroma samples of %d bytes' step)", L->uv_stride, cw * L->uv_step, L->uv_step);
        if (L->uv_step == 2 && std::llabs(L->u_offset - L->v_offset) != 1)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: interleaved chroma needs |v_offset - u_offset| == 1 (got %lld, %lld)",
                 (long long)L->u_offset, (long long)L->v_offset);
    } else {
        if (L->y_stride < bps * w)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: y_stride %d < 2 * width %d (16-bit containers: strides are bytes)", L->y_stride, w);
        if ((int64_t)L->uv_stride < (int64_t)bps * cw * L->uv_step)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: uv_stride %d < %d (width/2 chroma samples of 2 * %d bytes' step, 16-bit containers)",
                 L->uv_stride, bps * cw * L->uv_step, L->uv_step);
        if ((L->y_stride | L->uv_stride) & 1)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: 16-bit containers need even strides (y_stride %d, uv_stride %d)", L->y_stride, L->uv_stride);
        if ((L->u_offset | L->v_offset) & 1)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: 16-bit containers need even offsets (u_offset %lld, v_offset %lld)",
                 (long long)L->u_offset, (long long)L->v_offset);
        if (frame_stride >= 0 && (frame_stride & 1))
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420: 16-bit containers need an even frame_stride (%lld)", (long long)frame_stride);
        if (L->uv_step == 2 && std::llabs(L->u_offset - L->v_offset) != 2)
            fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: interleaved chroma of 16-bit containers needs |v_offset - u_offset| == 2 (got %lld, %lld)",
                 (long long)L->u_offset, (long long)L->v_offset);
    }
    // planes as byte ranges [lo, hi): Y, then U and V (one range when interleaved)
    const int64_t y_hi = (int64_t)(h - 1) * L->y_stride + (int64_t)w * bps;
    const int64_t c_rows = (int64_t)(ch - 1) * L->uv_stride;
    struct R { int64_t lo, hi; const char* name; };
    R pl[3] = {{0, y_hi, "Y"}, {0, 0, ""}, {0, 0, ""}};
    int npl;
    if (L->uv_step == 2) {
        const int64_t lo = std::min(L->u_offset, L->v_offset);
        pl[1] = R{lo, lo + c_rows + (int64_t)2 * cw * bps, "UV"};
        npl = 2;
    } else {
        pl[1] = R{L->u_offset, L->u_offset + c_rows + (int64_t)cw * bps, "U"};
        pl[2] = R{L->v_offset, L->v_offset + c_rows + (int64_t)cw * bps, "V"};
        npl = 3;
    }
    int64_t span = 0;
    for (int i = 0; i < npl; ++i) {
        span = std::max(span, pl[i].hi);
        for (int j = 0; j < i; ++j)
            if (pl[i].lo < pl[j].hi && pl[j].lo < pl[i].hi)
                fail(SLIDEO_ERR_INVALID_ARG, "yuv420 layout: the %s plane [%lld, %lld) overlaps the %s plane [%lld, %lld)", pl[i].name,
                     (long long)pl[i].lo, (long long)pl[i].hi, pl[j].name, (long long)pl[j].lo, (long long)pl[j].hi);
    }
    if (frame_stride >= 0 && frame_stride < span)
        fail(SLIDEO_ERR_INVALID_ARG, "yuv420: frame_stride %lld does not cover the frame's furthest byte (%lld)", (long long)frame_stride, (long long)span);
    return span;
}

// The layout rules of include/slideo_amd.h "YUV sampling": 4:2:2 (chroma (w/2) x h) and 4:4:4 (chroma w x h) in the record's own
// terms, and packed 4:2:2 (one plane of 4-byte macropixels).  Messages carry the sampling's name (yuv422 / yuv444 / yuv422 packed).
inline int64_t yuv_sampled_validate(int w, int h, const slideo_yuv420_layout* L, int64_t frame_stride, int bps, int sampling) {
    const bool packed = sampling == SLIDEO_YUV_SAMPLING_422_PACKED, s444 = sampling == SLIDEO_YUV_SAMPLING_444;
    const char* name = packed ? "yuv422 packed" : s444 ? "yuv444" : "yuv422";
    if (w < 1 || h < 1) fail(SLIDEO_ERR_INVALID_ARG, "bad image geometry w=%d h=%d", w, h);
    if (!s444 && (w & 1)) fail(SLIDEO_ERR_UNSUPPORTED, "%s: the width must be even (%dx%d): two pixels share a chroma sample", name, w, h);
    if (w > MAX_DIM || h > MAX_DIM) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", w, h, MAX_DIM);
    if (packed) {
        if (bps != 1) fail(SLIDEO_ERR_UNSUPPORTED, "%s: 8-bit samples only (SLIDEO_YUV_DEPTH_8)", name);
        if (L->uv_step != 4) fail(SLIDEO_ERR_INVALID_ARG, "%s layout: uv_step %d is not 4 (one macropixel of two pixels)", name, L->uv_step);
        if (L->uv_stride != L->y_stride)
            fail(SLIDEO_ERR_INVALID_ARG, "%s layout: uv_stride %d is not y_stride %d (there is one plane)", name, L->uv_stride, L->y_stride);
        if ((int64_t)L->y_stride < (int64_t)2 * w) fail(SLIDEO_ERR_INVALID_ARG, "%s layout: y_stride %d < 2 * width %d", name, L->y_stride, w);
        const int64_t u = L->u_offset, v = L->v_offset;
        if (!((u == 1 && v == 3) || (u == 3 && v == 1) || (u == 0 && v == 2) || (u == 2 && v == 0)))
            fail(SLIDEO_ERR_INVALID_ARG, "%s layout: (u_offset, v_offset) = (%lld, %lld) is none of (1, 3) YUY2, (3, 1) YVYU, (0, 2) UYVY, (2, 0) VYUY",
                 name, (long long)u, (long long)v);
        const int64_t span = (int64_t)(h - 1) * L->y_stride + (int64_t)2 * w;
        if (frame_stride >= 0 && frame_stride < span)
            fail(SLIDEO_ERR_INVALID_ARG, "%s: frame_stride %lld does not cover the frame's furthest byte (%lld)", name, (long long)frame_stride, (long long)span);
        return span;
    }
    if (L->uv_step != 1 && L->uv_step != 2) fail(SLIDEO_ERR_INVALID_ARG, "%s layout: uv_step %d is neither 1 (planar) nor 2 (interleaved)", name, L->uv_step);
    if (L->u_offset < 0 || L->v_offset < 0) fail(SLIDEO_ERR_INVALID_ARG, "%s layout: negative plane offset", name);
    const int cw = s444 ? w : w / 2;
    const char* cws = s444 ? "width" : "width/2";
    if ((int64_t)L->y_stride < (int64_t)bps * w) fail(SLIDEO_ERR_INVALID_ARG, "%s layout: y_stride %d < %d (width %d samples of %d bytes)", name, L->y_stride, bps * w, w, bps);
    if ((int64_t)L->uv_stride < (int64_t)bps * cw * L->uv_step)
        fail(SLIDEO_ERR_INVALID_ARG, "%s layout: uv_stride %d < %lld (%s chroma samples of %d bytes, step %d)", name, L->uv_stride,
             (long long)bps * cw * L->uv_step, cws, bps, L->uv_step);
    if (bps == 2) {
        if ((L->y_stride | L->uv_stride) & 1)
            fail(SLIDEO_ERR_INVALID_ARG, "%s layout: 16-bit containers need even strides (y_stride %d, uv_stride %d)", name, L->y_stride, L->uv_stride);
        if ((L->u_offset | L->v_offset) & 1)
            fail(SLIDEO_ERR_INVALID_ARG, "%s layout: 16-bit containers need even offsets (u_offset %lld, v_offset %lld)", name,
                 (long long)L->u_offset, (long long)L->v_offset);
        if (frame_stride >= 0 && (frame_stride & 1))
            fail(SLIDEO_ERR_INVALID_ARG, "%s: 16-bit containers need an even frame_stride (%lld)", name, (long long)frame_stride);
    }
    if (L->uv_step == 2 && std::llabs(L->u_offset - L->v_offset) != bps)
        fail(SLIDEO_ERR_INVALID_ARG, "%s layout: interleaved chroma needs |v_offset - u_offset| == %d (got %lld, %lld)", name, bps,
             (long long)L->u_offset, (long long)L->v_offset);
    // planes as byte ranges [lo, hi): Y, then U and V (one range when interleaved); chroma has h rows
    const int64_t y_hi = (int64_t)(h - 1) * L->y_stride + (int64_t)w * bps;
    const int64_t c_rows = (int64_t)(h - 1) * L->uv_stride;
    struct R { int64_t lo, hi; const char* name; };
    R pl[3] = {{0, y_hi, "Y"}, {0, 0, ""}, {0, 0, ""}};
    int npl;
    if (L->uv_step == 2) {
        const int64_t lo = std::min(L->u_offset, L->v_offset);
        pl[1] = R{lo, lo + c_rows + (int64_t)2 * cw * bps, "UV"};
        npl = 2;
    } else {
        pl[1] = R{L->u_offset, L->u_offset + c_rows + (int64_t)cw * bps, "U"};
        pl[2] = R{L->v_offset, L->v_offset + c_rows + (int64_t)cw * bps, "V"};
        npl = 3;
    }
    int64_t span = 0;
    for (int i = 0; i < npl; ++i) {
        span = std::max(span, pl[i].hi);
        for (int j = 0; j < i; ++j)
            if (pl[i].lo < pl[j].hi && pl[j].lo < pl[i].hi)
                fail(SLIDEO_ERR_INVALID_ARG, "%s layout: the %s plane [%lld, %lld) of %d rows overlaps the %s plane [%lld, %lld)", name, pl[i].name,
                     (long long)pl[i].lo, (long long)pl[i].hi, h, pl[j].name, (long long)pl[j].lo, (long long)pl[j].hi);
    }
    if (frame_stride >= 0 && frame_stride < span)
        fail(SLIDEO_ERR_INVALID_ARG, "%s: frame_stride %lld does not cover the frame's furthest byte (%lld)", name, (long long)frame_stride, (long long)span);
    return span;
}

// ---- frame lists (include/slideo_amd.h "Frame lists") ---------------------------------------------------------------------------------
// What a list's frames become in the library's own memory, the same for host and device lists: per frame `frame_bytes` bytes, staged
// plane j (n_planes of them) holding rows[j] rows of row_bytes[j] bytes packed tight at dst_ofs[j], read from the address
// planes[3i + k[j]] at rows src_stride[j] apart.  Interleaved chroma is ONE staged plane from the lower of the U and V addresses.
// The staged frames are what the contiguous twin takes: `yuv` (YUV door: the tight layout of the format class) or rows `stride`
// apart (BGR door; planar formats: every plane's), frames frame_bytes apart.
struct FrameListPlan {
    bool yuv_door = false;
    int n_planes = 0;
    int k[3] = {0, 0, 0}, rows[3] = {0, 0, 0};
    int64_t row_bytes[3] = {0, 0, 0}, src_stride[3] = {0, 0, 0}, dst_ofs[3] = {0, 0, 0};
    int64_t frame_bytes = 0;
    slideo_yuv420_layout yuv{};
    int stride = 0;
};

// The one host-side planning function of a list: every rule of "Frame lists" (each names itself), then the plan.  Nothing is written
// anywhere.  yuv, pixel_format: the matcher's (the list's door picks which is read).
inline FrameListPlan frame_list_plan(const slideo_frame_list* L, const YuvDesc& yuv, int pixel_format) {
    if (!L) fail(SLIDEO_ERR_INVALID_ARG, "frame list: null record");
    if (L->door != SLIDEO_FRAME_LIST_BGR && L->door != SLIDEO_FRAME_LIST_YUV)
        fail(SLIDEO_ERR_INVALID_ARG, "frame list: door %d is neither SLIDEO_FRAME_LIST_BGR (0) nor SLIDEO_FRAME_LIST_YUV (1)", L->door);
    if (L->on_device != 0 && L->on_device != 1) fail(SLIDEO_ERR_INVALID_ARG, "frame list: on_device %d is neither 0 (host) nor 1 (device)", L->on_device);
    if (L->n_frames < 0) fail(SLIDEO_ERR_INVALID_ARG, "frame list: n_frames %d is negative", L->n_frames);
    if (L->n_frames > 0 && !L->planes) fail(SLIDEO_ERR_INVALID_ARG, "frame list: null planes array");
    const int w = L->width, h = L->height, n = L->n_frames;
    const uint8_t* const* A = reinterpret_cast<const uint8_t* const*>(L->planes);
    FrameListPlan P;
    P.yuv_door = L->door == SLIDEO_FRAME_LIST_YUV;
    int bps = 1;
    bool paired = false;                             // interleaved or packed: stride[1], stride[2] repeat another plane's
    if (P.yuv_door) {
        bps = yuv.bytes_per_sample();
        const bool packed = yuv.sampling == SLIDEO_YUV_SAMPLING_422_PACKED;
        if (packed ? L->uv_step != 4 : (L->uv_step != 1 && L->uv_step != 2))
            fail(SLIDEO_ERR_INVALID_ARG, "frame list: uv_step %d is not one the sampling %d has (%s)", L->uv_step, yuv.sampling,
                 packed ? "4: one macropixel of two pixels" : "1: planar, 2: interleaved");
        // the U / V order (interleaved) or the offset pair (packed) of the list: frame 0's, which every frame must repeat (below)
        int64_t du = packed ? 1 : 0, dv = packed ? 3 : bps;
        if (n > 0 && A[0] && A[1] && A[2]) {
            if (packed) { du = A[1] - A[0]; dv = A[2] - A[0]; }
            else if (L->uv_step == 2) { du = A[1] < A[2] ? 0 : bps; dv = A[1] < A[2] ? bps : 0; }
        }
        const int cw = yuv.sampling == SLIDEO_YUV_SAMPLING_444 ? w : w / 2, ch = yuv.sampling == SLIDEO_YUV_SAMPLING_420 ? h / 2 : h;
        const int64_t luma = (int64_t)bps * w * h, chroma = (int64_t)bps * cw * ch;
        slideo_yuv420_layout& T = P.yuv;
        T.uv_step = L->uv_step;
        if (packed) { T.y_stride = T.uv_stride = 2 * w; T.u_offset = du; T.v_offset = dv; }
        else {
            T.y_stride = bps * w; T.uv_stride = bps * cw * L->uv_step;
            T.u_offset = L->uv_step == 2 ? luma + du : luma;
            T.v_offset = L->uv_step == 2 ? luma + dv : luma + chroma;
        }
        // the door's size rules and image limits with their codes and messages (and, packed, its offset-pair rule) on the tight layout
        P.frame_bytes = yuv420_validate(w, h, &T, -1, bps, yuv.sampling);
        paired = packed || L->uv_step == 2;
        P.n_planes = packed ? 1 : L->uv_step == 2 ? 2 : 3;
        P.rows[0] = h; P.row_bytes[0] = packed ? (int64_t)2 * w : (int64_t)bps * w;
        for (int j = 1; j < P.n_planes; ++j) {
            P.k[j] = L->uv_step == 2 ? (du == 0 ? 1 : 2) : j;
            P.rows[j] = ch; P.row_bytes[j] = (int64_t)bps * cw * L->uv_step;
            P.dst_ofs[j] = luma + (j - 1) * chroma;
        }
    } else {
        int bpp = 0, planes = 0;
        if (!pixel_format_info(pixel_format, &bpp, &planes)) fail(SLIDEO_ERR_INVALID_ARG, "pixel format: %d is not a format", pixel_format);
        if (w < 1 || h < 1) fail(SLIDEO_ERR_INVALID_ARG, "bad image geometry w=%d h=%d", w, h);
        if ((int64_t)bpp * w > INT32_MAX) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", w, h, MAX_DIM);
        P.stride = bpp * w;
        P.n_planes = planes;
        for (int j = 0; j < planes; ++j) { P.k[j] = j; P.rows[j] = h; P.row_bytes[j] = (int64_t)bpp * w; P.dst_ofs[j] = (int64_t)j * h * P.stride; }
        P.frame_bytes = (int64_t)planes * h * P.stride;
    }
    // strides: of every plane the door reads
    const int nread = P.yuv_door ? 3 : P.n_planes;
    for (int k = 0; k < nread; ++k) {
        const int j = paired ? (P.n_planes == 1 ? 0 : std::min(k, 1)) : k;       // the staged plane whose rows plane k's stride steps over
        if (L->stride[k] < 0) fail(SLIDEO_ERR_INVALID_ARG, "frame list: stride[%d] %lld is negative (flipped frames are not supported)", k, (long long)L->stride[k]);
        if (L->stride[k] < P.row_bytes[j])
            fail(SLIDEO_ERR_INVALID_ARG, "frame list: stride[%d] %lld < the plane's row bytes %lld", k, (long long)L->stride[k], (long long)P.row_bytes[j]);
        if (bps == 2 && (L->stride[k] & 1)) fail(SLIDEO_ERR_INVALID_ARG, "frame list: 16-bit containers need even strides (stride[%d] %lld)", k, (long long)L->stride[k]);
    }
    if (paired && L->stride[1] != L->stride[2])
        fail(SLIDEO_ERR_INVALID_ARG, "frame list: %s chroma needs stride[1] == stride[2] (got %lld, %lld)", P.n_planes == 1 ? "packed" : "interleaved",
             (long long)L->stride[1], (long long)L->stride[2]);
    if (paired && P.n_planes == 1 && L->stride[1] != L->stride[0])
        fail(SLIDEO_ERR_INVALID_ARG, "frame list: packed frames have one plane: stride[1] %lld is not stride[0] %lld", (long long)L->stride[1], (long long)L->stride[0]);
    for (int j = 0; j < P.n_planes; ++j) P.src_stride[j] = L->stride[P.k[j]];
    // addresses: of every frame
    for (int i = 0; i < n; ++i) {
        const uint8_t* const* a = A + 3 * (int64_t)i;
        for (int k = 0; k < 3; ++k) {
            if (k < nread && !a[k]) fail(SLIDEO_ERR_INVALID_ARG, "frame list: frame %d: plane %d is needed and NULL", i, k);
            if (k >= nread && a[k]) fail(SLIDEO_ERR_INVALID_ARG, "frame list: frame %d: plane %d is not read under this format and not NULL", i, k);
            if (bps == 2 && ((uintptr_t)a[k] & 1)) fail(SLIDEO_ERR_INVALID_ARG, "frame list: frame %d: 16-bit containers need even addresses (plane %d)", i, k);
        }
        if (!paired) continue;
        if (P.n_planes == 1) {
            if (a[1] - a[0] != P.yuv.u_offset || a[2] - a[0] != P.yuv.v_offset)
                fail(SLIDEO_ERR_INVALID_ARG, "frame list: frame %d: packed planes at (%lld, %lld) past the frame, frame 0's valid pair is (%lld, %lld)", i,
                     (long long)(a[1] - a[0]), (long long)(a[2] - a[0]), (long long)P.yuv.u_offset, (long long)P.yuv.v_offset);
        } else {
            const int64_t d = a[2] - a[1];
            if (d != bps && d != -bps)
                fail(SLIDEO_ERR_INVALID_ARG, "frame list: frame %d: interleaved chroma needs planes[3i+2] - planes[3i+1] == +-%d (got %lld)", i, bps, (long long)d);
            if ((d > 0) != (P.k[1] == 1))
                fail(SLIDEO_ERR_INVALID_ARG, "frame list: frame %d: interleaved chroma in another U / V order than frame 0's", i);
        }
    }
    return P;
}

// ---- the rules between settings (SLIDEO_ERR_UNSUPPORTED), each once --------------------------------------------------------------
// `next`: the settings in force with the proposed change of `what` applied.  The settings in force keep every rule, so the call
// that would complete a refused combination fails, and the values before stay in force.
inline void frame_settings_rules(const FrameSettings& next, Setting what, bool sift_on) {
    // no mask in SIFT mode (clearing one is always allowed)
    if (what == SET_FRAME_MASK && next.mask.set && sift_on)
        fail(SLIDEO_ERR_UNSUPPORTED, "the frame mask filters ORB's FAST candidates: not in SIFT mode");
    // a region's output fits the working size
    const FrameRegion& R = next.region;
    if (R.set && next.work_w > 0 && (R.out_w > next.work_w || R.out_h > next.work_h))
        fail(SLIDEO_ERR_UNSUPPORTED, "%s: the frame region's output %dx%d exceeds the working size %dx%d: a region's output must fit the working size",
             what == SET_WORKING_SIZE ? "working size" : "frame region", R.out_w, R.out_h, next.work_w, next.work_h);
    // a lens and a region describe the same source frames; a lens alone is a rectifying call of its own source size, which must fit
    // the working size (the source is exempt, as for the region); the radial map is strictly increasing over the reach, whichever of
    // the two set calls changes the reach
    const FrameLens& L = next.lens;
    if (L.set && R.set && (L.src_w != R.src_w || L.src_h != R.src_h))
        fail(SLIDEO_ERR_UNSUPPORTED, "the frame lens's source size %dx%d is not the frame region's source size %dx%d: both describe the same frames",
             L.src_w, L.src_h, R.src_w, R.src_h);
    if (L.set && !R.set && next.work_w > 0 && (L.src_w > next.work_w || L.src_h > next.work_h))
        fail(SLIDEO_ERR_UNSUPPORTED, "%s: a frame lens without a region analyses frames at its source size %dx%d, which exceeds the working size %dx%d "
             "(a lens counts as a rectifying call: its output must fit the working size)", what == SET_WORKING_SIZE ? "working size" : "frame lens",
             L.src_w, L.src_h, next.work_w, next.work_h);
    if (L.set && (what == SET_FRAME_REGION || what == SET_WORKING_SIZE)) {
        const double R2 = frame_lens_reach(L, R);
        if (!frame_lens_monotone(L.k1, L.k2, R2))
            fail(SLIDEO_ERR_INVALID_ARG, "frame lens: the radial map r (1 + k1 r^2 + k2 r^4) with k1 %g, k2 %g is not strictly increasing over the reach "
                 "r^2 <= %g of the %s's corners (1 + 3 k1 s + 5 k2 s^2 > 0 over 0 <= s <= r^2)", L.k1, L.k2, R2, R.set ? "frame region" : "source frame");
    }
    // a direct similarity compares whole small images: not beside a mask the gate compares under, unless the look-up does too
    if (next.direct_t > 0.f && next.gate_scope() && next.direct_scope != SLIDEO_DIRECT_VALID)
        fail(SLIDEO_ERR_UNSUPPORTED, "the direct page look-up compares whole small images: not together with a frame mask under SLIDEO_MASK_GATE "
             "(a look-up over the valid pixels only: slideo_matcher_set_direct_scope(m, SLIDEO_DIRECT_VALID))");
    // a gate settle defers frames that are away from the ANCHOR: it means nothing under PREVIOUS
    if (next.settle_similarity > 0.f && next.gate_ref != SLIDEO_GATE_ANCHOR)
        fail(SLIDEO_ERR_UNSUPPORTED, "gate settle under SLIDEO_GATE_ANCHOR only: a settle similarity %g with the gate reference SLIDEO_GATE_PREVIOUS "
             "(slideo_matcher_set_gate_reference(m, SLIDEO_GATE_ANCHOR) first; slideo_matcher_set_gate_settle(m, 0, 0) before going back)",
             (double)next.settle_similarity);
    // a gate memory recalls frames that are away from the ANCHOR: it means nothing under PREVIOUS
    if (next.gate_memory > 0 && next.gate_ref != SLIDEO_GATE_ANCHOR)
        fail(SLIDEO_ERR_UNSUPPORTED, "gate memory under SLIDEO_GATE_ANCHOR only: a capacity of %d with the gate reference SLIDEO_GATE_PREVIOUS "
             "(slideo_matcher_set_gate_reference(m, SLIDEO_GATE_ANCHOR) first; slideo_matcher_set_gate_memory(m, 0) before going back)",
             next.gate_memory);
    // packed 4:2:2 is 8-bit: whichever of the two set calls (sampling, description) would complete the pair is refused
    if (next.yuv.sampling == SLIDEO_YUV_SAMPLING_422_PACKED && next.yuv.depth != SLIDEO_YUV_DEPTH_8)
        fail(SLIDEO_ERR_UNSUPPORTED, "SLIDEO_YUV_SAMPLING_422_PACKED reads 8-bit samples: not together with a 10-bit depth (%d); packed 10-bit "
             "formats (Y210, v210) are not supported", next.yuv.depth);
    // a transfer reads 10-bit samples in full: whichever of the two set calls (transfer, description) would complete the pair is refused
    if (next.yuv.transfer != SLIDEO_YUV_TRANSFER_SDR && next.yuv.depth == SLIDEO_YUV_DEPTH_8)
        fail(SLIDEO_ERR_UNSUPPORTED, "a YUV transfer (%d) reads 10-bit samples: not together with SLIDEO_YUV_DEPTH_8 (and so not with "
             "SLIDEO_YUV_SAMPLING_422_PACKED, which is 8-bit); slideo_matcher_set_yuv_description with a 10-bit depth first", next.yuv.transfer);
    // bilinear chroma under a transfer is out of scope: whichever of the three set calls (transfer, chroma filter, sampling) would
    // complete the combination is refused
    if (next.yuv.transfer != SLIDEO_YUV_TRANSFER_SDR && next.yuv.filtered())
        fail(SLIDEO_ERR_UNSUPPORTED, "a YUV transfer (%d) together with the chroma filter %d under sampling %d: bilinear chroma under a transfer "
             "is out of scope (SLIDEO_YUV_CHROMA_NEAREST, or 4:4:4 frames)", next.yuv.transfer, next.yuv.chroma, next.yuv.sampling);
}

}  // namespace slideo
