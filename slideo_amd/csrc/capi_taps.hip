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

// The unit from the frames' features on: the caller's keypoints and descriptors in place of ORB's output (unit_submit_sift is the
// model: rows made elsewhere into the common search and verify stages).  One unit on slot 0, the exact-size search, no pipelining.
int32_t slideo_match_frames_features_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                          int32_t stride_bytes, int64_t frame_stride_bytes, const int32_t* kp_counts,
                                          const slideo_keypoint* kp, const uint8_t* desc32, slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (m->sift_on) fail(SLIDEO_ERR_INVALID_ARG, "frame features are 32-byte ORB descriptors: not in SIFT mode");
    if (m->cfg.matcher != 0) fail(SLIDEO_ERR_INVALID_ARG, "frame features go through the exact Hamming search only (matcher 0)");
    const int n = n_frames;
    FrameSrc src = FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes);
    validate_frames(src, m, n, verdicts_out);
    if (src.plan.prep != PREP_NONE) fail(SLIDEO_ERR_INVALID_ARG, "frame features belong to the frames as given: not under a working size or a frame region");
    if (n > 4096) fail(SLIDEO_ERR_INVALID_ARG, "at most 4096 frames in one call");
    if (n > 0 && !kp_counts) fail(SLIDEO_ERR_INVALID_ARG, "null kp_counts");
    std::vector<uint32_t> qofs((size_t)n + 1, 0);
    uint32_t mx = 0;
    for (int i = 0; i < n; ++i) {
        if (kp_counts[i] < 0 || (int64_t)qofs[i] + kp_counts[i] >= ((int64_t)1 << 30)) fail(SLIDEO_ERR_INVALID_ARG, "bad keypoint count of frame %d", i);
        qofs[i + 1] = qofs[i] + (uint32_t)kp_counts[i];
        mx = std::max(mx, (uint32_t)kp_counts[i]);
    }
    const uint32_t qtot = qofs[n];
    if (qtot > 0 && (!kp || !desc32)) fail(SLIDEO_ERR_INVALID_ARG, "null keypoints/descriptors");
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    m->last_fcs.clear();
    if (n == 0) return SLIDEO_OK;
    evidence_admit(m, width, height, n);
    tone_admit(m, n);
    placement_admit(m, width, height, n);
    shading_map_admit(m, width, height, n);
    // (a failure from here on may leave rows counted whose verdicts are never returned: an open evidence session ends with it)
    struct EvidenceGuard { slideo_matcher* m; bool ok; ~EvidenceGuard() { if (!ok) sessions_drop(m); } } ev_guard{m, false};
    area_class_for(m, width, height);
    upload_area(m);
    const slideo_config& c = m->cfg;
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    const size_t tail = (size_t)n * (sizeof(slideo_verdict) + sizeof(FrameCands));
    for (;;) {
        S.knn.shared = false; S.gate.on = false; S.u_set = m->cur_set; S.u_rerun = false;
        const DevFrames f = stage_frames(m, S, src, 0, n);
        S.timed = false; S.u_in = f; S.u_mask = nullptr; S.u_async = false;
        S.orb.qofs = qofs; S.orb.qtot = qtot; S.orb.max_count = mx; S.orb.nframes = n;
        S.d_kp.reserve(std::max<size_t>((size_t)qtot * sizeof(slideo_keypoint), 16));
        S.d_desc.reserve(std::max<size_t>((size_t)qtot * 32, 32));
        S.d_qofs.reserve((size_t)(n + 1) * 4 + 16); S.d_info.reserve(64); S.d_flags.reserve(16);
        S.h_info.reserve((size_t)(n + 1) * 4 + 16);
        uint32_t* hq = S.h_info.as<uint32_t>();
        std::memcpy(hq, qofs.data(), (size_t)(n + 1) * 4);
        hq[n + 1] = qtot; hq[n + 2] = mx;
        if (qtot > 0) {
            HIP_CHECK(hipMemcpyAsync(S.d_kp.p, kp, (size_t)qtot * sizeof(slideo_keypoint), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(S.d_desc.p, desc32, (size_t)qtot * 32, hipMemcpyHostToDevice, st));
        }
        HIP_CHECK(hipMemcpyAsync(S.d_qofs.p, hq, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(S.d_info.p, hq + n + 1, 8, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(S.d_flags.p, 0, 16, st));
        knn_plan_unit(m, S, n, (int64_t)f.w * f.h, qtot, qtot);
        S.d_votes.reserve(std::max<size_t>((size_t)qtot * c.knn_k * sizeof(uint2), 16));
        S.d_gpts.reserve(std::max<size_t>((size_t)qtot * c.knn_k * sizeof(float4), 16));
        S.d_gmask.reserve(std::max<size_t>((size_t)qtot * c.knn_k, 16));
        S.d_fcs.reserve((size_t)n * sizeof(FrameCands));
        S.d_verdicts.reserve((size_t)n * sizeof(slideo_verdict));
        S.d_pairs.reserve((size_t)n * MAXR * sizeof(PairDesc) + 64);
        S.h_out.reserve(tail + 64);
        HIP_CHECK(hipMemsetAsync(S.d_fcs.p, 0, (size_t)n * sizeof(FrameCands), st));
        VerifyParams vp = make_vp(c);
        vp.rng_len = m->rng_len;
        if (qtot > 0) unit_knn(m, S, n, qtot, qtot, false, false);
        unit_verify(m, S, vp, f, n, qtot);
        HIP_CHECK(hipStreamSynchronize(st));
        S.busy = false;
        uint32_t fl;
        std::memcpy(&fl, S.h_out.as<uint8_t>() + tail, 4);
        if (!(fl & 4u)) break;
        // a candidate's sample schedule ran past the pre-drawn stream (unit_collect's rule, without its re-run through ORB): draw
        // four times as much and run these rows again
        const uint32_t cap = 1u << 26;
        if (m->rng_len >= cap) fail(SLIDEO_ERR_CAPACITY, "RANSAC sample schedule exceeded %u pre-drawn RNG outputs", m->rng_len);
        HIP_CHECK(hipDeviceSynchronize());
        upload_rng_stream(m, (uint32_t)std::min<uint64_t>((uint64_t)m->rng_len * 4, cap));
    }
    const uint8_t* ho = S.h_out.as<uint8_t>();
    std::memcpy(verdicts_out, ho, (size_t)n * sizeof(slideo_verdict));
    evidence_tally(m, verdicts_out, n);
    tone_tally(m, n);
    placement_tally(m, n);
    shading_map_tally(m, n);
    ev_guard.ok = true;
    m->last_fcs.resize((size_t)n);
    std::memcpy(m->last_fcs.data(), ho + (size_t)n * sizeof(slideo_verdict), (size_t)n * sizeof(FrameCands));
    API_CATCH(m)
}

// Tap: the length of the pre-drawn cv::RNG stream now (it starts at SLIDEO_RNG_STREAM_LEN and grows when a unit outran it and was run again)
int32_t slideo_matcher_rng_stream_len(const slideo_matcher* m, int64_t* len) {
    if (!m || !len) return SLIDEO_ERR_INVALID_ARG;
    *len = (int64_t)m->rng_len;
    return SLIDEO_OK;
}

int32_t slideo_yuv420_to_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height, const slideo_yuv420_layout* layout,
                              uint8_t* bgr_out, int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!frame || !bgr_out) fail(SLIDEO_ERR_INVALID_ARG, "null frame/bgr_out");
    FrameSrc img = FrameSrc::yuv420(frame, false, width, height, layout, -1);
    img.describe(m->fs);
    img.levels = img.shading = false;               // (the conversion's image: the shading and the levels come behind it, slideo_levels_bgr8)
    validate_frames(img);
    const size_t fb = (size_t)width * height * 3;
    if ((int64_t)fb > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the BGR image needs %zu bytes", fb);
    tap_staged(m, img, bgr_out, (int64_t)fb);
    API_CATCH(m)
}

}  // extern "C"
