// capi_taps.hip — debug taps of the parity tests (no kernel of its own).
#include "runtime.hpp"

using namespace slideo;

extern "C" {

// ---- debug taps ---------------------------------------------------------------------------

int32_t slideo_orb_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes,
                        slideo_keypoint* kp, uint8_t* desc32, int32_t capacity, int32_t* n_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !n_out) fail(SLIDEO_ERR_INVALID_ARG, "null image/n_out");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    // an image of the frame mask's size is analysed as a frame of that size is: under the mask
    const uint8_t* mask_pyr = (m->fs.mask.set && width == m->fs.mask.w && height == m->fs.mask.h) ? frame_mask_for(m, width, height) : nullptr;
    run_orb(m, S, stage_frames(m, S, img, 0, 1), 1, false, false, mask_pyr);
    const uint32_t q = S.orb.qtot;
    *n_out = (int32_t)q;
    if ((int64_t)q > capacity) fail(SLIDEO_ERR_CAPACITY, "%u keypoints, capacity %d", q, capacity);
    if (q) {
        if (kp) HIP_CHECK(hipMemcpyAsync(kp, S.d_kp.p, (size_t)q * sizeof(slideo_keypoint), hipMemcpyDeviceToHost, st));
        if (desc32) HIP_CHECK(hipMemcpyAsync(desc32, S.d_desc.p, (size_t)q * 32, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    API_CATCH(m)
}

int32_t slideo_pyramid_level_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes,
                                  int32_t level, int32_t blurred, uint8_t* out, int64_t out_capacity, int32_t* lw, int32_t* lh) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !out || !lw || !lh) fail(SLIDEO_ERR_INVALID_ARG, "null argument");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    if (level < 0 || level >= m->cfg.nlevels) fail(SLIDEO_ERR_INVALID_ARG, "level out of range");
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    run_orb(m, S, stage_frames(m, S, img, 0, 1), 1, false, blurred != 0);
    const LevelGeom& L = geom_for(m, width, height).g.lv[level];
    *lw = L.w; *lh = L.h;
    if ((int64_t)L.w * L.h > out_capacity) fail(SLIDEO_ERR_CAPACITY, "level needs %lld bytes", (long long)L.w * L.h);
    if (L.w > 0 && L.h > 0) {
        const uint8_t* src = (blurred ? S.d_blur.as<uint8_t>() : S.d_pyr.as<uint8_t>()) + L.ofs;
        HIP_CHECK(hipMemcpy2DAsync(out, L.w, src, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    API_CATCH(m)
}

int32_t slideo_frame_mask_level(slideo_matcher* m, int32_t level, uint8_t* out, int64_t out_capacity, int32_t* lw, int32_t* lh) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!out || !lw || !lh) fail(SLIDEO_ERR_INVALID_ARG, "null argument");
    if (!m->fs.mask.set) fail(SLIDEO_ERR_STATE, "no frame mask is set");
    if (level < 0 || level >= m->cfg.nlevels) fail(SLIDEO_ERR_INVALID_ARG, "level out of range");
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    const LevelGeom& L = geom_for(m, m->fs.mask.w, m->fs.mask.h).g.lv[level];
    *lw = L.w; *lh = L.h;
    if ((int64_t)L.w * L.h > out_capacity) fail(SLIDEO_ERR_CAPACITY, "level needs %lld bytes", (long long)L.w * L.h);
    if (L.w > 0 && L.h > 0) {
        HIP_CHECK(hipMemcpy2DAsync(out, L.w, m->d_mask_pyr.as<uint8_t>() + L.ofs, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, m->stream));
        HIP_CHECK(hipStreamSynchronize(m->stream));
    }
    API_CATCH(m)
}

int32_t slideo_frame_mask_small(slideo_matcher* m, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh, int64_t* n_valid) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!sw || !sh || !n_valid) fail(SLIDEO_ERR_INVALID_ARG, "null sw/sh/n_valid");
    if (!m->fs.mask.set) fail(SLIDEO_ERR_STATE, "no frame mask is set");
    if (!m->fs.gate_map.on)
        fail(SLIDEO_ERR_STATE, "the frame mask's scope lacks SLIDEO_MASK_GATE: there is no validity map (slideo_matcher_set_frame_mask_scope)");
    require_idle(m);
    const GateMap& g = m->fs.gate_map;
    *sw = g.sw; *sh = g.sh; *n_valid = g.n_valid;
    const int64_t npx = (int64_t)g.sw * g.sh;
    if (out && npx > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the validity map needs %lld bytes", (long long)npx);
    if (out) {
        HIP_CHECK(hipSetDevice(m->device));
        std::vector<uint8_t> w((size_t)npx * 3);
        HIP_CHECK(hipMemcpyAsync(w.data(), m->d_gate_w.p, w.size(), hipMemcpyDeviceToHost, m->stream));
        HIP_CHECK(hipStreamSynchronize(m->stream));
        for (int64_t i = 0; i < npx; ++i) out[i] = w[(size_t)i * 3];      // (a pixel's three weight bytes are equal)
    }
    API_CATCH(m)
}

int32_t slideo_small_image_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes,
                                uint8_t* out, int64_t out_capacity, int32_t* sw_out, int32_t* sh_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !out || !sw_out || !sh_out) fail(SLIDEO_ERR_INVALID_ARG, "null argument");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    int sw = 0, sh = 0;
    run_small(m, stage_frames(m, S, img, 0, 1), 1, st, &sw, &sh);
    *sw_out = sw; *sh_out = sh;
    if ((int64_t)sw * sh * 3 > out_capacity) fail(SLIDEO_ERR_CAPACITY, "small image needs %lld bytes", (long long)sw * sh * 3);
    HIP_CHECK(hipMemcpyAsync(out, m->d_small.p, (size_t)sw * sh * 3, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    API_CATCH(m)
}

int32_t slideo_yuv420_to_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height, const slideo_yuv420_layout* layout,
                              uint8_t* bgr_out, int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!frame || !bgr_out) fail(SLIDEO_ERR_INVALID_ARG, "null frame/bgr_out");
    FrameSrc img = FrameSrc::yuv420(frame, false, width, height, layout, -1);
    img.describe(m->fs.yuv);
    validate_frames(img);
    const size_t fb = (size_t)width * height * 3;
    if ((int64_t)fb > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the BGR image needs %zu bytes", fb);
    tap_staged(m, img, bgr_out, (int64_t)fb);
    API_CATCH(m)
}

}  // extern "C"
