// frame_settings.h — the frame settings of a matcher as ONE record (include/slideo_amd.h "Working size", "Frame region", "Frame mask",
// "Frame mask scope", "Direct page look-up", "Direct look-up scope"): the record, every setter's proposal with its range checks, the
// rules between settings, what a change of each ends.  Plain C++, no HIP include (tools/frame_settings_hostcheck.cpp walks it on the
// host); the device buffers a setting owns are the matcher's (runtime.hpp).  A change takes ONE path: settings_commit (capi_runtime.hip).
#pragma once
#include <cmath>
#include <cstdint>

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
// A w x h mask; frames of that analysed size keep only the FAST candidates its pyramid (the matcher's d_mask_pyr) allows
struct FrameMask { bool set = false; int w = 0, h = 0; };
// The gate's validity map, in force while a mask is set under SLIDEO_MASK_GATE: one weight byte (0xFF valid, 0x00) per byte of the
// sw x sh small image of frames of the mask's size (the matcher's d_gate_w), n_valid valid pixels
struct GateMap { bool on = false; int sw = 0, sh = 0; int64_t n_valid = 0; };

struct FrameSettings {
    int work_w = 0, work_h = 0;                       // frames beyond it are reduced in front of the pipeline; 0, 0 = none
    FrameRegion region;                               // frames of region.src_w x src_h stand for their rectified image
    FrameMask mask;
    uint32_t mask_scope = SLIDEO_MASK_DETECT;         // SLIDEO_MASK_DETECT | SLIDEO_MASK_GATE; the matcher's, whatever happens to the mask
    GateMap gate_map;
    uint64_t gate_map_gen = 1;                        // what is derived from the map (the look-up's masked page norms) is cached under it
    float direct_t = 0.f;                             // the direct similarity (0: off)
    uint32_t direct_scope = SLIDEO_DIRECT_WHOLE;      // VALID = the look-up over the gate's valid pixels
    bool gate_scope() const { return mask.set && (mask_scope & SLIDEO_MASK_GATE); }      // the gate compares under the mask
};

enum Setting { SET_WORKING_SIZE, SET_FRAME_REGION, SET_FRAME_MASK, SET_FRAME_MASK_SCOPE, SET_DIRECT_SIMILARITY, SET_DIRECT_SCOPE, N_SETTINGS };

// What a change of each setting ends: the frames a mask call kept (made under the earlier setting), the gate state (so was its small
// image; under a mask change it stays: it is a whole frame's), the map's generation.  Applied by settings_commit and, the group's
// half, by group_set: nowhere else.
struct SettingEnds { bool kept, gate, map_gen; };
constexpr SettingEnds SETTING_ENDS[N_SETTINGS] = {{true, true, true}, {true, true, false}, {true, false, true}, {true, false, true},
                                                  {false, false, false}, {false, false, false}};

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
    // a direct similarity compares whole small images: not beside a mask the gate compares under, unless the look-up does too
    if (next.direct_t > 0.f && next.gate_scope() && next.direct_scope != SLIDEO_DIRECT_VALID)
        fail(SLIDEO_ERR_UNSUPPORTED, "the direct page look-up compares whole small images: not together with a frame mask under SLIDEO_MASK_GATE "
             "(a look-up over the valid pixels only: slideo_matcher_set_direct_scope(m, SLIDEO_DIRECT_VALID))");
}

}  // namespace slideo
