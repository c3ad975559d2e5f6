// capi_runtime.hip — handles, page database, workspace slots, unit submit / collect and the match entry points of include/slideo_amd.h (no kernel of its own).
#include "runtime.hpp"
#include "shading_field.h"
#include <chrono>

using namespace slideo;

namespace slideo {

namespace {
std::string g_create_error;
std::mutex g_err_mutex;
}

void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) fail(SLIDEO_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
}

GeomEntry& geom_for(slideo_matcher* m, int w, int h) {
    for (auto& g : m->geoms) if (g->w == w && g->h == h) return *g;
    if (w < 1 || h < 1 || w > MAX_DIM || h > MAX_DIM)
        fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", w, h, MAX_DIM);
    auto e = std::make_unique<GeomEntry>();
    e->w = w; e->h = h;
    std::vector<uint32_t> tab;
    build_pyr_geom(w, h, m->cfg, e->g, tab);
    orb_geom_init(m, *e, tab);
    m->geoms.push_back(std::move(e));
    return *m->geoms.back();
}

int area_class_for(slideo_matcher* m, int w, int h) {
    for (size_t i = 0; i < m->area_geoms.size(); ++i)
        if (m->area_geoms[i].sw == w && m->area_geoms[i].sh == h) return (int)i;
    AreaGeom a;
    if (!build_area_geom(w, h, m->cfg.small_area, a, m->area_taps, m->area_idx, m->cfg.ocv.area, &m->area_recs))
        fail(SLIDEO_ERR_UNSUPPORTED, "image %dx%d has area below small_area=%d: to_small_image would upscale (INTER_AREA falls back to bilinear in OpenCV), not implemented",
             w, h, m->cfg.small_area);
    m->area_geoms.push_back(a);
    m->area_dirty = true;
    return (int)m->area_geoms.size() - 1;
}

void upload_area(slideo_matcher* m) {
    if (!m->area_dirty) return;
    m->d_area_geoms.reserve(m->area_geoms.size() * sizeof(AreaGeom));
    m->d_area_taps.reserve(m->area_taps.size() * sizeof(AreaTap));
    m->d_area_idx.reserve(m->area_idx.size() * 4);
    m->d_area_recs.reserve(std::max<size_t>(m->area_recs.size() * sizeof(AreaRec), 64));
    HIP_CHECK(hipMemcpyAsync(m->d_area_geoms.p, m->area_geoms.data(), m->area_geoms.size() * sizeof(AreaGeom), hipMemcpyHostToDevice, m->stream));
    HIP_CHECK(hipMemcpyAsync(m->d_area_taps.p, m->area_taps.data(), m->area_taps.size() * sizeof(AreaTap), hipMemcpyHostToDevice, m->stream));
    HIP_CHECK(hipMemcpyAsync(m->d_area_idx.p, m->area_idx.data(), m->area_idx.size() * 4, hipMemcpyHostToDevice, m->stream));
    if (!m->area_recs.empty()) HIP_CHECK(hipMemcpyAsync(m->d_area_recs.p, m->area_recs.data(), m->area_recs.size() * sizeof(AreaRec), hipMemcpyHostToDevice, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    m->area_dirty = false;
}

// max frames of size (w,h) per unit under the workspace budget (the slots share it)
int sub_batch_for(slideo_matcher* m, const PyrGeom& g, int n, size_t staging, size_t fixed) {
    size_t per = (size_t)g.frame_bytes * (blur_is_f32(m) ? 2 : 1) + (size_t)g.cand_per_frame * 4 + (size_t)g.nlevels * 258 * 4 + (size_t)g.w * g.h * 3;
    per += staging;          // the 4:2:0 staging in front of the BGR image, the source-sized frames of a reducing call (other calls keep their unit sizes)
    // downstream of ORB, sized by the per-frame keypoint capacity: items 8 + keypoint 24 + descriptor 32 B, the key lists
    // (32 x 4 B, times the train-set segments of a small query set: at most ~4 at sizes where the budget matters), and per
    // (keypoint, neighbour) the vote 8 B + point pair 16 B + mask 1 B
    const size_t kc = kp_cap_for(m, g);
    per += kc * (8 + sizeof(slideo_keypoint) + 32 + (size_t)KLIST * 4 * 4 + (size_t)m->cfg.knn_k * 25) + sizeof(FrameCands) + MAXR * sizeof(PairDesc);
    // fixed: what a unit takes whatever its frame count (the gate memory's ring and operand), out of the slot's share first
    const size_t share = m->ws_budget / NSLOTS;
    size_t fit = std::max<size_t>(1, (share - std::min(fixed, share)) / std::max<size_t>(per, 1));
    return (int)std::min<size_t>({(size_t)std::max(n, 1), fit, (size_t)4096});
}

void require_idle(slideo_matcher* m) {
    for (const Slot& S : m->slots) if (S.busy) fail(SLIDEO_ERR_STATE, "a submitted unit has not been collected yet");
}

// page-locked (hipHostMalloc / hipHostRegister) host memory?  Copies from it are truly asynchronous DMA; copies from pageable
// memory are staged by the runtime inside the call.
static bool host_is_pinned(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

void validate_image(int w, int h, int stride) {
    if (w < 1 || h < 1 || stride < w * 3) fail(SLIDEO_ERR_INVALID_ARG, "bad image geometry w=%d h=%d stride=%d", w, h, stride);
}

void validate_frames(FrameSrc& src, slideo_matcher* m, int n, const void* out) {
    if (m) src.describe(m->fs);                                    // (a call without a matcher argument here sets it itself)
    if (src.yuv) {
        src.yuv_span = yuv420_validate(src.w, src.h, src.yuv, src.frame_stride, src.bps, src.sampling);
        src.stride = src.w * 3;                                    // the BGR image the units read (d_stage)
    } else if (src.pixel_format != SLIDEO_PIXEL_BGR8 && src.src_stride == 0) {
        src.pix_span = pixel_format_validate(src.pixel_format, src.w, src.h, src.stride, src.frame_stride);
        src.src_stride = src.stride;
        src.stride = src.w * 3;                                    // likewise
    }
    if (m) {
        if (!m->finalized) fail(SLIDEO_ERR_STATE, "slideo_matcher_finalize_pages must be called before matching");
        if (m->M <= 0) fail(SLIDEO_ERR_EMPTY_INDEX, "no page produced a descriptor");
        if (n < 0 || (n > 0 && (!src.p || !out))) fail(SLIDEO_ERR_INVALID_ARG, "null frames/verdicts");
    }
    validate_image(src.w, src.h, src.stride);
    if (m) resolve_frames(m, src, true);
    if (m && !src.converted() && src.frame_stride < (int64_t)src.h * src.stride) fail(SLIDEO_ERR_INVALID_ARG, "frame_stride smaller than one frame");
    src.pinned = !src.on_device && src.p && host_is_pinned(src.p);
    // (a list counts as pinned iff every frame's first plane is)
    if (src.list && src.pinned)
        for (int i = 1; i < src.list_count() && src.pinned; ++i) src.pinned = host_is_pinned(src.list_planes(i)[0]);
}

// A list's frames [first, first + n) into the plan's staged layout at dst (frames P.frame_bytes apart).  Host lists: one copy per
// plane on st — one span where the plane's stride is its row bytes, else one 2-D copy; interleaved chroma from the lower of the U and
// V addresses.  Device lists: the unit's addresses into the slot's table, then frame_gather_kernel on the slot's stream.
static void stage_list(Slot& S, const FrameSrc& src, int first, int n, uint8_t* dst, hipStream_t st) {
    const FrameListPlan& P = src.list->plan;
    const uint8_t* const* a = src.list_planes(first);
    if (src.on_device) {
        S.u_list = src.list;                            // (the addresses stay the library's until the slot's next list unit)
        S.d_ltab.reserve((size_t)n * 3 * sizeof(void*) + 16);
        // (the library's copy of the addresses is pageable: the runtime has staged it when the call returns)
        HIP_CHECK(hipMemcpyAsync(S.d_ltab.p, a, (size_t)n * 3 * sizeof(void*), hipMemcpyHostToDevice, S.st));
        launch_frame_gather(P, S.d_ltab.as<const uint8_t*>(), n, dst, S.st);
        return;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < P.n_planes; ++j) {
            const uint8_t* s = a[3 * (size_t)i + P.k[j]];
            uint8_t* d = dst + P.frame_bytes * i + P.dst_ofs[j];
            const size_t rb = (size_t)P.row_bytes[j];
            if (P.src_stride[j] == P.row_bytes[j]) HIP_CHECK(hipMemcpyAsync(d, s, rb * (size_t)P.rows[j], hipMemcpyHostToDevice, st));
            else HIP_CHECK(hipMemcpy2DAsync(d, rb, s, (size_t)P.src_stride[j], rb, (size_t)P.rows[j], hipMemcpyHostToDevice, st));
        }
}

// prep, unit size and small size: the frame region, else the working size (the region's output fits it: the set calls' rule)
void resolve_unit(const slideo_matcher* m, FrameSrc& src, bool with_lens) {
    const FrameSettings& fs = m->fs;
    const FrameRegion& R = fs.region;
    const FrameLens& L = fs.lens;
    const bool lens = L.set && with_lens;
    const int small_area = m->cfg.small_area;
    if ((R.set || lens) && !src.analysed) {
        if (R.set && (src.w != R.src_w || src.h != R.src_h))
            fail(SLIDEO_ERR_INVALID_ARG, "frame size %dx%d is not the frame region's source size %dx%d", src.w, src.h, R.src_w, R.src_h);
        if (lens && (src.w != L.src_w || src.h != L.src_h))
            fail(SLIDEO_ERR_INVALID_ARG, "frame size %dx%d is not the frame lens's source size %dx%d", src.w, src.h, L.src_w, L.src_h);
        // (a lens without a region: a rectifying call of its own source size, which fits the working size — the set calls' rule)
        src.plan.unit(PREP_RECTIFY, R.set ? R.out_w : L.src_w, R.set ? R.out_h : L.src_h, small_area);
        src.plan.lens = lens;
    } else if (fs.work_w > 0 && (src.w > fs.work_w || src.h > fs.work_h)) {
        int rw = 0, rh = 0;
        working_size_rule(src.w, src.h, fs.work_w, fs.work_h, rw, rh);
        src.plan.unit(PREP_REDUCE, rw, rh, small_area);
    } else src.plan.unit(PREP_NONE, src.w, src.h, small_area);
    // (a frame shading holds frames of its own analysed size only, as a frame mask does: refused before anything is touched)
    const FrameShading& F = fs.shading;
    if (src.shading && (src.plan.uw != F.aw || src.plan.uh != F.ah))
        fail(SLIDEO_ERR_INVALID_ARG, "frames analysed at %dx%d under a frame shading of %dx%d (slideo_matcher_set_frame_shading)", src.plan.uw, src.plan.uh,
             F.aw, F.ah);
}

void resolve_frames(const slideo_matcher* m, FrameSrc& src, bool match) {
    FramePlan& P = src.plan;
    resolve_unit(m, src);
    if (match) {
        if (P.prep == PREP_REDUCE && (src.w > MAX_DIM || src.h > MAX_DIM)) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", src.w, src.h, MAX_DIM);
        if (m->sift_on) sift_check_cfg(&m->sift_cfg, P.uw, P.uh);              // (the doubled image's coordinates travel in 13 bits)
        if (m->cur_set != 0) page_set_check_mode(m);                          // (a mode switched on after slideo_matcher_use_page_set)
        P.mask_pyr = frame_mask_for(m, P.uw, P.uh);                           // (a frame mask holds frames of its own size only)
    }
    // (under the frame mask's GATE scope the flags are the mask's: frames of another analysed size are an error, before anything is touched)
    P.gate_w = gate_map_for(m, P.uw, P.uh, P.sw, P.sh, &P.npx);
}

void settings_commit(slideo_matcher* m, Setting what, FrameSettings next, const uint8_t* mask, int stride) {
    const bool masks = what == SET_FRAME_MASK || what == SET_FRAME_MASK_SCOPE;
    if (masks) HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    frame_settings_rules(next, what, m->sift_on);
    if (what == SET_FRAME_REGION && next.region.set) frame_region_classify(next.region);
    // a new mask's pyramid and, under the GATE scope, the validity map of the mask in force (level 0 of the pyramid: the mask as
    // given) come first: a mask whose map is refused leaves the mask before in force
    DevBuf pyr, map_w;
    const bool new_mask = what == SET_FRAME_MASK && next.mask.set;
    if (new_mask) frame_mask_build(m, mask, next.mask.w, next.mask.h, stride, pyr);
    if (masks && !next.gate_scope()) next.gate_map = GateMap{};
    else if (masks && (new_mask || !next.gate_map.on)) {
        const LevelGeom& L0 = geom_for(m, next.mask.w, next.mask.h).g.lv[0];
        gate_map_build(m, (new_mask ? pyr : m->d_mask_pyr).as<uint8_t>() + L0.ofs, L0.pitch, next.mask.w, next.mask.h, next.gate_map, map_w);
    }
    if (new_mask) m->d_mask_pyr = std::move(pyr);
    if (map_w.p) m->d_gate_w = std::move(map_w);
    // a new levels table's device copy (the matcher is idle: no kernel is reading the one before)
    if (next.levels.set && (!m->fs.levels.set || std::memcmp(next.levels.lut, m->fs.levels.lut, 768) != 0)) {
        HIP_CHECK(hipSetDevice(m->device));
        m->d_levels.reserve(768);
        HIP_CHECK(hipMemcpy(m->d_levels.p, next.levels.lut, 768, hipMemcpyHostToDevice));
    }
    // a new gain field's device copy (likewise; the nodes are shared, so another pointer is another field)
    if (next.shading.set && next.shading.gains != m->fs.shading.gains) {
        HIP_CHECK(hipSetDevice(m->device));
        const size_t bytes = next.shading.gains->size() * sizeof(uint16_t);
        m->d_shading.reserve(bytes);
        HIP_CHECK(hipMemcpy(m->d_shading.p, next.shading.gains->data(), bytes, hipMemcpyHostToDevice));
    }
    // a new transfer's tables (likewise)
    if (next.yuv.transfer != SLIDEO_YUV_TRANSFER_SDR && (next.yuv.transfer != m->fs.yuv.transfer || next.yuv.white_nits != m->fs.yuv.white_nits)) {
        std::vector<uint8_t> tab(2 * YUV_TR_LIN + YUV_TR_OUT);
        std::vector<uint16_t> lin(YUV_TR_LIN);
        yuv_transfer_lin_out(next.yuv.transfer, (double)next.yuv.white_nits, lin.data(), tab.data() + 2 * YUV_TR_LIN);
        std::memcpy(tab.data(), lin.data(), 2 * YUV_TR_LIN);
        HIP_CHECK(hipSetDevice(m->device));
        m->d_transfer.reserve(tab.size());
        HIP_CHECK(hipMemcpy(m->d_transfer.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    }
    m->fs = next;
    const SettingEnds& ends = SETTING_ENDS[what];
    if (ends.kept) m->kept.valid = false;
    if (ends.kept && ends.gate) sessions_drop(m);      // (the analysed image changes under an open evidence or tone session: the state "none")
    if (ends.gate) { gate_state_reset(m); m->gate_refs.clear(); m->gate_refs_valid = false; }
    if (ends.map_gen) ++m->fs.gate_map_gen;
}

// S's staging buffer with room for `bytes`.  Slot 0's holds the frames slideo_changed_mask_bgr8 kept for slideo_match_kept_frames:
// whatever the mask call left there is overwritten (any slot's, as a call's units cycle through them all)
uint8_t* stage_for_upload(slideo_matcher* m, Slot& S, size_t bytes) {
    m->kept.valid = false;
    S.d_stage.reserve(bytes + 16);
    return S.d_stage.as<uint8_t>();
}

DevFrames stage_frames(slideo_matcher* m, Slot& S, const FrameSrc& src, int first, int n, hipStream_t cs, DevBuf* into) {
    const uint8_t* p = src.list ? nullptr : src.p + (int64_t)first * src.frame_stride;
    const FramePlan& P = src.plan;      // (a tap's unresolved plan is PREP_NONE: uw, uh are read under `pre` alone)
    const bool pre = P.prep != PREP_NONE;                        // a kernel stands between the BGR view at source size and the unit's image
    if (src.on_device && !src.kernel_in_front()) return DevFrames{p, src.w, src.h, src.stride, src.frame_stride};
    const int uw = P.uw, uh = P.uh;
    const int64_t fb = (int64_t)src.h * src.stride;              // one frame of the BGR view at source size (stride 3w for YUV frames)
    const int64_t ub = pre ? (int64_t)uh * uw * 3 : fb;          // one frame of the unit's BGR image
    uint8_t* stage;
    if (into) { into->reserve((size_t)ub * n + 16); stage = into->as<uint8_t>(); }
    else stage = stage_for_upload(m, S, (size_t)ub * n);
    int64_t fs = src.frame_stride;
    if (src.list) {
        // a frame list, host or device: into the staged layout where a host frame's upload goes, and a host-frame unit from there on
        uint8_t* dst = stage;
        fs = src.list->plan.frame_bytes;                // (a single frame's frame_stride may be -1)
        if (src.converted() || pre) { S.d_yuv.reserve((size_t)fs * n + 16); dst = S.d_yuv.as<uint8_t>(); }
        stage_list(S, src, first, n, dst, !src.on_device && cs ? cs : S.st);
        if (!src.on_device && cs) {
            HIP_CHECK(hipEventRecord(S.ev_up, cs));
            HIP_CHECK(hipStreamWaitEvent(S.st, S.ev_up, 0));
        }
        p = dst;
    } else if (!src.on_device) {
        // host frames back to back into d_stage, or into d_yuv for the conversion / the reduce / the rectify below
        const int64_t bytes = src.converted() ? src.src_span() : fb;
        uint8_t* dst = stage;
        if (src.converted() || pre) { S.d_yuv.reserve((size_t)bytes * n + 16); dst = S.d_yuv.as<uint8_t>(); }
        hipStream_t st = cs ? cs : S.st;
        if (fs == bytes) {
            HIP_CHECK(hipMemcpyAsync(dst, p, (size_t)bytes * n, hipMemcpyHostToDevice, st));
        } else {
            for (int i = 0; i < n; ++i)
                HIP_CHECK(hipMemcpyAsync(dst + bytes * i, p + fs * i, (size_t)bytes, hipMemcpyHostToDevice, st));
        }
        if (cs) {
            HIP_CHECK(hipEventRecord(S.ev_up, cs));
            HIP_CHECK(hipStreamWaitEvent(S.st, S.ev_up, 0));
        }
        p = dst; fs = bytes;
    }
    // 4:2:0 frames: converted on the slot's stream into its d_stage, which lives until the unit is collected (verify's re-projection
    // reads the frames); into d_full when the image is reduced or rectified next (both come after convert)
    // frames of another pixel format: the same, device frames out of the caller's memory
    if (src.converted()) {
        uint8_t* bgr = stage;
        if (pre) { S.d_full.reserve((size_t)fb * n + 16); bgr = S.d_full.as<uint8_t>(); }
        if (src.yuv) launch_yuv420_to_bgr(m->fs.yuv, p, fs, *src.yuv, src.w, src.h, n, bgr, S.st, m->d_transfer.as<uint32_t>());
        else launch_pixels_to_bgr(src.pixel_format, p, fs, src.src_stride, src.w, src.h, n, bgr, S.st);
        p = bgr; fs = fb;
    }
    // frame levels: the last step in front of the unit, in place on the staged image — but plain device BGR frames, which nothing has
    // staged yet, out of the caller's memory (never written) into the stage, rows as far apart as the caller's
    // frame shading: in front of the levels, by the same rule; with both set ONE pass does both (shading_kernel's fused instance)
    if (!pre) {
        if (src.shading) launch_shading(m, src.levels, p, fs, src.stride, stage, fb, src.stride, src.w, src.h, n, S.st);
        else if (src.levels) launch_levels(m, p, fs, src.stride, stage, fb, src.stride, src.w, src.h, n, S.st);
        return DevFrames{stage, src.w, src.h, src.stride, fb};
    }
    if (P.prep == PREP_RECTIFY) launch_rectify(m->fs.region, P.lens ? &m->fs.lens : nullptr, p, fs, src.stride, n, stage, S.st);
    else launch_reduce(m, p, fs, src.stride, src.w, src.h, uw, uh, n, stage, S.st);
    if (src.shading) launch_shading(m, src.levels, stage, ub, uw * 3, stage, ub, uw * 3, uw, uh, n, S.st);
    else if (src.levels) launch_levels(m, stage, ub, uw * 3, stage, ub, uw * 3, uw, uh, n, S.st);
    return DevFrames{stage, uw, uh, uw * 3, ub};
}

void tap_staged(slideo_matcher* m, const FrameSrc& img, uint8_t* out, int64_t ob) {
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    HIP_CHECK(hipMemcpyAsync(out, stage_frames(m, S, img, 0, 1).p, (size_t)ob, hipMemcpyDeviceToHost, S.st));
    HIP_CHECK(hipStreamSynchronize(S.st));
}

// the cv::RNG((uint64)-1) stream RANSACPointSetRegistrator draws its samples from, pre-drawn (ptsetreg.cpp: rng state
// starts at -1 on every call, so every candidate reads the same stream from position 0)
void upload_rng_stream(slideo_matcher* m, uint32_t len) {
    std::vector<uint32_t> rng(len);
    CvRng r((uint64_t)-1, m->cfg.ocv.rng_mul);
    for (auto& v : rng) v = r.next();
    m->d_rng.reserve(rng.size() * 4);
    HIP_CHECK(hipMemcpy(m->d_rng.p, rng.data(), rng.size() * 4, hipMemcpyHostToDevice));
    m->rng_len = len;
}

// keypoints per frame the capacity-sized path provides for: twice the quota (ties at a level's retainBest threshold are kept, so
// no finite bound is safe; a frame beyond it is detected on the device and the unit re-run through the exact-size path)
uint32_t kp_cap_for(const slideo_matcher* m, const PyrGeom& g) {
    int cap = std::max(2 * m->cfg.nfeatures, m->cfg.nfeatures + 1024);
    cap = std::min(cap, KP_SORT_LDS);
    return (uint32_t)std::max(1, std::min(cap, std::max(g.cand_per_frame, 1)));
}

// ---- one unit of the per-frame hot path: enqueue everything, then collect ---------------
// `f` must stay valid until the unit is collected (reproject reads the frames).
void unit_submit(slideo_matcher* m, Slot& S, const DevFrames& f, int n, const uint8_t* mask_pyr, bool allow_async) {
    // (does this unit share the chip with others?  the search then runs one block per CU: stage_knn.hip knn_plan)
    { bool others = m->units_pending; for (const Slot& o : m->slots) others |= (&o != &S && o.busy); S.knn.shared = others; }
    S.gate.on = false;                             // (a gated unit: stage_gate.hip marks it after this submit)
    if (!S.u_rerun) S.u_set = m->cur_set;          // (a re-run of an overflowed unit searches the set it was submitted with)
    S.u_rerun = false;
    if (m->sift_on) { unit_submit_sift(m, S, f, n); return; }
    const slideo_config& c = m->cfg;
    hipStream_t st = S.st;
    const bool prof = m->profiling;
    const PyrGeom& g = geom_for(m, f.w, f.h).g;
    // Capacity-sized (no host wait in the middle of the unit) when the matrix-core kNN runs: every kernel downstream of the ORB
    // counts reads them on the device.  The VALU engine (A/B only) keeps the exact-size path.
    const uint32_t kpcap = kp_cap_for(m, g);
    // (a capacity below quota + margin — the KP_SORT_LDS clamp at nfeatures >= ~7 k — would overflow on every busy frame and run
    // every unit twice: those configurations take the exact-size path from the start)
    const bool async = allow_async && m->async_submit && !knn_unit_is_valu(m) &&
                       (int64_t)n * kpcap < ((int64_t)1 << 30) &&
                       (kpcap >= (uint32_t)c.nfeatures + 1024u || kpcap >= (uint32_t)std::max(g.cand_per_frame, 1));
    S.timed = prof; S.u_in = f; S.u_mask = mask_pyr; S.u_async = async;
    if (m->orb_chain && m->last_orb_ev && m->last_orb_ev != S.ev_orb) HIP_CHECK(hipStreamWaitEvent(st, m->last_orb_ev, 0));
    if (prof) HIP_CHECK(hipEventRecord(S.ev[0], st));
    orb_stage1(m, S, f, n, false, async ? kpcap : 0xFFFFFFFFu, mask_pyr);      // (a re-run applies the mask again)
    uint32_t qtot, qplan;
    if (async) {
        qtot = (uint32_t)n * kpcap;                                          // capacity
        qplan = (uint32_t)n * std::min<uint32_t>(kpcap, (uint32_t)c.nfeatures);   // what the kNN plan assumes
        S.orb.qtot = qtot; S.orb.max_count = kpcap;
    } else {
        orb_wait_info(m, S);                  // the other units' kNN / verify keep the GPU busy meanwhile
        qtot = qplan = S.orb.qtot;
    }
    // all workspace before the timed kNN interval
    knn_plan_unit(m, S, n, (int64_t)f.w * f.h, qplan, qtot);
    S.d_votes.reserve(std::max<size_t>((size_t)qtot * c.knn_k * sizeof(uint2), 16));
    S.d_gpts.reserve(std::max<size_t>((size_t)qtot * c.knn_k * sizeof(float4), 16));
    S.d_gmask.reserve(std::max<size_t>((size_t)qtot * c.knn_k, 16));
    S.d_fcs.reserve((size_t)n * sizeof(FrameCands));
    S.d_verdicts.reserve((size_t)n * sizeof(slideo_verdict));
    S.d_pairs.reserve((size_t)n * MAXR * sizeof(PairDesc) + 64);
    S.h_out.reserve((size_t)n * (sizeof(slideo_verdict) + sizeof(FrameCands)) + 64);
    orb_stage2(m, S, f.w, f.h, async);
    HIP_CHECK(hipEventRecord(S.ev_orb, st));
    m->last_orb_ev = S.ev_orb;
    VerifyParams vp = make_vp(c);
    vp.rng_len = m->rng_len;
    HIP_CHECK(hipMemsetAsync(S.d_fcs.p, 0, (size_t)n * sizeof(FrameCands), st));
    if (prof) HIP_CHECK(hipEventRecord(S.ev[1], st));
    if (qtot > 0) unit_knn(m, S, n, qplan, qtot, async, prof);      // (records S.ev[2] behind the search when profiling)
    unit_verify(m, S, vp, f, n, qtot);
}

static void unit_collect_body(slideo_matcher* m, Slot& S, slideo_verdict* out_host);
// (a collect that fails — a HIP error, an overflow that cannot be served — may leave a unit counted whose verdicts are never
// returned: an open evidence session ends with it)
void unit_collect(slideo_matcher* m, Slot& S, slideo_verdict* out_host) {
    try { unit_collect_body(m, S, out_host); }
    catch (...) { sessions_drop(m); throw; }
}

static void unit_collect_body(slideo_matcher* m, Slot& S, slideo_verdict* out_host) {
    const int n = S.n;
    HIP_CHECK(hipStreamSynchronize(S.st));
    S.busy = false;
    const uint8_t* ho = S.h_out.as<uint8_t>();
    const size_t tail = (size_t)n * (sizeof(slideo_verdict) + sizeof(FrameCands));
    uint32_t fl, info[2];
    std::memcpy(&fl, ho + tail, 4);
    std::memcpy(info, ho + tail + 4, 8);
    if (S.u_async) {
        if (fl & 1u) fail(SLIDEO_ERR_HIP, "internal: FAST candidate list overflow");
        if (fl & 8u) {
            // a frame had more keypoints than the capacity-sized path provides for (ties at a retainBest threshold are kept, as
            // in OpenCV): the whole unit again, through the exact-size path
            S.u_rerun = true;
            unit_submit(m, S, S.u_in, n, S.u_mask, false);
            unit_collect(m, S, out_host);
            return;
        }
        S.orb.qtot = info[0]; S.orb.max_count = info[1];
    }
    const uint32_t qtot = S.orb.qtot;
    if (fl & 4u) {
        // a candidate's sample schedule (2 draws per iteration + the redraws of equal pairs; 4 per attempt for the homography) ran
        // past the pre-drawn stream: draw four times as much and run the unit again.  (Other units may be reading the table:
        // drain the device first.)
        const uint32_t cap = 1u << 26;
        if (m->rng_len >= cap) fail(SLIDEO_ERR_CAPACITY, "RANSAC sample schedule exceeded %u pre-drawn RNG outputs", m->rng_len);
        HIP_CHECK(hipDeviceSynchronize());
        upload_rng_stream(m, (uint32_t)std::min<uint64_t>((uint64_t)m->rng_len * 4, cap));
        S.u_rerun = true;
        unit_submit(m, S, S.u_in, n, S.u_mask, false);
        unit_collect(m, S, out_host);
        return;
    }
    if (S.timed) {                    // (after both re-run checks: a unit that was run twice is counted once, by its final run)
        float t;
        HIP_CHECK(hipEventElapsedTime(&t, S.ev[0], S.ev[1])); m->prof_ms[0] += t; m->prof_n[0]++;
        if (qtot > 0) {
            HIP_CHECK(hipEventElapsedTime(&t, S.ev[1], S.ev[2])); m->prof_ms[1] += t; m->prof_n[1]++;
            m->prof_pairs += (int64_t)qtot * S.knn.nt;       // pairs EVALUATED: unique train rows when the set is de-duplicated
            HIP_CHECK(hipEventElapsedTime(&t, S.ev[2], S.ev[3])); m->prof_ms[2] += t; m->prof_n[2]++;
        }
        HIP_CHECK(hipEventElapsedTime(&t, S.ev[0], S.ev[4])); m->prof_ms[3] += t; m->prof_n[3]++;
    }
    std::memcpy(out_host, ho, (size_t)n * sizeof(slideo_verdict));
    tone_tally(m, n);
    placement_tally(m, n);
    shading_map_tally(m, n);
    evidence_tally(m, out_host, n);                  // (the run whose verdicts are returned: evidence_kernel counted this one alone)
    const size_t base = m->last_fcs.size();
    m->last_fcs.resize(base + n);
    std::memcpy(m->last_fcs.data() + base, ho + (size_t)n * sizeof(slideo_verdict), (size_t)n * sizeof(FrameCands));
}

// A unit of either kind begun on slot S: frames [first, first + n) of src staged and, plain, all of them through unit_submit;
// gated, through the gate and the changed ones through unit_submit (stage_gate.hip)
static void unit_begin(slideo_matcher* m, Slot& S, const FrameSrc& src, int first, int n, hipStream_t cs, bool gated) {
    if (gated) gate_unit_submit(m, S, src, first, n, cs);
    else unit_submit(m, S, stage_frames(m, S, src, first, n, cs), n, src.plan.mask_pyr);
}

// max frames per unit of a call of either kind under the workspace budget
static int unit_fit(slideo_matcher* m, const FrameSrc& src, int n, bool gated) {
    const int fit = sub_batch_for(m, geom_for(m, src.plan.uw, src.plan.uh).g, n, src.staging_bytes(gated ? gate_small_budget(m) : 0),
                                  gated ? gate_memory_budget(m) : 0);
    // (under SLIDEO_GATE_ANCHOR a gated unit's pair table caps it: include/slideo_amd.h "Gate reference")
    return gated && m->fs.gate_ref == SLIDEO_GATE_ANCHOR ? std::min(fit, GATE_ANCHOR_MAX_UNIT) : fit;
}

// Synchronous matching of n frames, plain or gated (changed_out, similarity_out: a gated call's): cut into units and run them
// through the slots as a pipeline.
void match_frames_impl(slideo_matcher* m, int n, FrameSrc src, slideo_verdict* out, hipStream_t user_stream, bool gated, uint8_t* changed_out,
                       float* similarity_out) {
    if (gated && n > 0 && !changed_out) fail(SLIDEO_ERR_INVALID_ARG, "null changed_out");
    validate_frames(src, m, n, out);
    if (gated) gate_check(m->gate, src);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    m->last_fcs.clear();
    if (n == 0) return;
    evidence_admit(m, src.plan.uw, src.plan.uh, n);
    tone_admit(m, n);
    placement_admit(m, src.plan.uw, src.plan.uh, n);
    shading_map_admit(m, src.plan.uw, src.plan.uh, n);
    int unit = unit_fit(m, src, n, gated);
    area_class_for(m, src.plan.uw, src.plan.uh);
    upload_area(m);
    if (n >= 128 && unit >= (n + 1) / 2) unit = (n + 1) / 2;      // two halves overlap ORB with kNN / verify
    // Host frames: the call is bound by the H2D copies (6.2 MB per 1080p frame: 256 frames = 29 ms at 55 GB/s against 14 ms of
    // kernels), so what matters is that the copy engines never wait: short units, each copied (and, in a gated call, gated) on its
    // slot's stream while the units before it compute — with two halves the second half's kernels start only when all of it has arrived.
    if (!src.on_device && m->host_unit > 0 && n >= 2 * m->host_unit) unit = std::min(unit, m->host_unit);
    struct Pending { Slot* S; int ofs; };
    std::vector<Pending> pend;
    if (src.on_device && user_stream)
        for (Slot& S : m->slots) {      // inputs produced on the caller's stream: order our streams behind it
            HIP_CHECK(hipEventRecord(S.ev_in, user_stream));
            HIP_CHECK(hipStreamWaitEvent(S.st, S.ev_in, 0));
        }
    int done = 0;
    // pinned source: asynchronous copies, kept in submission order on the one copy stream (see copy_st); pageable source: the
    // runtime stages the copy inside the call, on the unit's own stream (measured: 32.7 ms per 256 frames that way against 54.8
    // through the copy stream)
    hipStream_t cs = src.pinned ? m->copy_st : nullptr;
    m->units_pending = n > unit;
    // with a gate memory the call's units append their refs in order ("Gate memory": slideo_matcher_last_gate_refs)
    struct RefsCall { slideo_matcher* m; ~RefsCall() { m->gate_refs_call = false; } } refs_call{m};
    if (gated && m->fs.gate_ref == SLIDEO_GATE_ANCHOR && m->fs.gate_memory > 0) { m->gate_refs.clear(); m->gate_refs_call = true; }
    auto collect = [&](const Pending& p) {
        if (gated) {
            gate_unit_collect(m, *p.S, changed_out + p.ofs, similarity_out ? similarity_out + p.ofs : nullptr, out + p.ofs);
            done += p.S->gate.n;
        } else {
            unit_collect(m, *p.S, out + p.ofs);
            done += p.S->n;
        }
        if (m->progress) m->progress(m->progress_user, (uint64_t)done, (uint64_t)n, "Processing frames...");
    };
    try {
        for (int i = 0; i < n; i += unit) {
            if ((int)pend.size() == NSLOTS) { collect(pend[0]); pend.erase(pend.begin()); }
            Slot& S = m->slots[m->next_slot];
            m->next_slot = (m->next_slot + 1) % NSLOTS;
            unit_begin(m, S, src, i, std::min(unit, n - i), cs, gated);
            pend.push_back({&S, i});
            // a chained group call: the state behind the call's last unit goes to the successor while this member's pipeline runs on
            if (gated && i + unit >= n && m->gate_publish) m->gate_publish(S);
        }
        for (Pending& p : pend) collect(p);
        m->units_pending = false;
    } catch (...) {
        m->units_pending = false;
        (void)hipStreamSynchronize(m->copy_st);          // (DMA from the caller's pinned buffer may still be running)
        for (Slot& S : m->slots) { (void)hipStreamSynchronize(S.st); S.busy = false; S.gate.on = false; }
        sessions_drop(m);                                // (units of the call may have counted: an open evidence or tone session ends)
        throw;
    }
}

// slideo_match_frames_submit[_yuv420]_dev and their gated twins: one unit admitted to the next slot
static void submit_impl(slideo_matcher* m, int32_t n_frames, FrameSrc src, void* hip_stream, int64_t* ticket_out, bool gated) {
    if (!ticket_out) fail(SLIDEO_ERR_INVALID_ARG, "null ticket_out");
    validate_frames(src, m, n_frames, ticket_out);
    if (n_frames < 1) fail(SLIDEO_ERR_INVALID_ARG, "submit needs at least one frame");
    if (gated) gate_check(m->gate, src);
    HIP_CHECK(hipSetDevice(m->device));
    Slot& S = m->slots[m->next_slot];
    if (S.busy) fail(SLIDEO_ERR_STATE, "all slots are in flight: collect ticket %lld first", (long long)S.ticket);
    const int fit = unit_fit(m, src, n_frames, gated);
    if (n_frames > fit)
        fail(SLIDEO_ERR_CAPACITY, "%d frames exceed the per-slot workspace budget (%d); submit smaller units or raise SLIDEO_WS_GB", n_frames, fit);
    evidence_admit(m, src.plan.uw, src.plan.uh, n_frames);
    tone_admit(m, n_frames);
    placement_admit(m, src.plan.uw, src.plan.uh, n_frames);
    shading_map_admit(m, src.plan.uw, src.plan.uh, n_frames);
    area_class_for(m, src.plan.uw, src.plan.uh);
    upload_area(m);
    { bool any = false; for (const Slot& c : m->slots) any |= c.busy; if (!any) m->last_fcs.clear(); }
    if (hip_stream) {
        HIP_CHECK(hipEventRecord(S.ev_in, reinterpret_cast<hipStream_t>(hip_stream)));
        HIP_CHECK(hipStreamWaitEvent(S.st, S.ev_in, 0));
    }
    try { unit_begin(m, S, src, 0, n_frames, nullptr, gated); }
    catch (...) { sessions_drop(m); throw; }      // (a unit half submitted may count: an open evidence or tone session ends)
    S.ticket = m->next_ticket++;
    *ticket_out = S.ticket;
    m->next_slot = (m->next_slot + 1) % NSLOTS;
    // the next units find their workspace sized (S.n = 0: a gated unit none of whose frames changed, which ran no pipeline)
    if (S.n > 0)
        for (Slot& O : m->slots) if (&O != &S && !O.busy) O.match_capacity(S);
}

// The slot whose unit a collect call of the given kind collects: in flight, the oldest ticket in flight, and of that kind
static Slot& slot_of_ticket(slideo_matcher* m, int64_t ticket, bool gated) {
    Slot* S = nullptr;
    for (Slot& c : m->slots) if (c.busy && c.ticket == ticket) S = &c;
    if (!S) fail(SLIDEO_ERR_STATE, "ticket %lld is not in flight", (long long)ticket);
    for (Slot& c : m->slots) if (c.busy && c.ticket < ticket) fail(SLIDEO_ERR_STATE, "collect ticket %lld first (in order)", (long long)c.ticket);
    if (S->gate.on && !gated) fail(SLIDEO_ERR_STATE, "ticket %lld is a gated unit: slideo_match_changed_frames_collect collects it", (long long)ticket);
    if (!S->gate.on && gated) fail(SLIDEO_ERR_STATE, "ticket %lld is not a gated unit: slideo_match_frames_collect collects it", (long long)ticket);
    return *S;
}

// slideo_changed_mask_bgr8 / _yuv420
void changed_mask_impl(slideo_matcher* m, int n_frames, FrameSrc src, const uint8_t* prev_small, uint8_t* last_small_out, uint8_t* changed_out,
                       float* similarity_out) {
    if (n_frames < 0 || (n_frames > 0 && (!src.p || !changed_out))) fail(SLIDEO_ERR_INVALID_ARG, "null frames/changed");
    src.describe(m->fs);
    validate_frames(src);
    resolve_frames(m, src, false);
    if (n_frames == 0) return;
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    const DevFrames f = stage_frames(m, S, src, 0, n_frames);
    m->kept = slideo_matcher::Kept{true, n_frames, f.w, f.h, f.stride};      // stays in slot 0's staging buffer: slideo_match_kept_frames
    run_small(m, f, n_frames, st);
    const size_t sb = (size_t)src.plan.sw * src.plan.sh * 3;
    const int npx = src.plan.npx;
    const uint8_t* weights = src.plan.gate_w;
    DevBuf& prev = m->d_prev_small;
    prev.reserve(sb);
    if (prev_small) HIP_CHECK(hipMemcpyAsync(prev.p, prev_small, sb, hipMemcpyHostToDevice, st));
    m->d_ssd.reserve((size_t)n_frames * 8);
    // pair i: (small[i-1], small[i]); pair 0 uses prev
    if (prev_small) launch_gate_ssd(weights, prev.as<uint8_t>(), 0, m->d_small.as<uint8_t>(), 0, (int64_t)sb, m->d_ssd.as<unsigned long long>(), 1, st);
    if (n_frames > 1)
        launch_gate_ssd(weights, m->d_small.as<uint8_t>(), (int64_t)sb, m->d_small.as<uint8_t>() + sb, (int64_t)sb, (int64_t)sb, m->d_ssd.as<unsigned long long>() + 1, n_frames - 1, st);
    std::vector<unsigned long long> ssd(n_frames, 0);
    HIP_CHECK(hipMemcpyAsync(ssd.data(), m->d_ssd.p, (size_t)n_frames * 8, hipMemcpyDeviceToHost, st));
    if (last_small_out)
        HIP_CHECK(hipMemcpyAsync(last_small_out, m->d_small.as<uint8_t>() + sb * (n_frames - 1), sb, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i < n_frames; ++i) {
        float sim = 0.0f;   // video_capture.rs:92: the first frame compares as 0.0
        if (i > 0 || prev_small) sim = changed_similarity(ssd[i], npx);
        changed_out[i] = sim < m->cfg.changed_similarity ? 1 : 0;
        if (similarity_out) similarity_out[i] = sim;
    }
}

// ProcessedImage::compute (mo/lib.rs:92-131) over n host pages: ORB (or SIFT) + to_small_image, runs of equally sized pages
// batched; the analysed pages, in order, into `out` (not appended to the matcher: the N-device group analyses a share of the
// deck on every device and appends the whole deck everywhere).  Progress: one report per page, (base + i + 1) of `total`.
void analyse_pages(slideo_matcher* m, int n_pages, const uint8_t* const* data, const int32_t* width, const int32_t* height, const int32_t* stride_bytes,
                   std::vector<HostPage>& out, uint64_t progress_base, uint64_t progress_total) {
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    int i = 0;
    while (i < n_pages) {
        // group a run of equally sized pages into one batch
        const int w = width[i], h = height[i], stride = stride_bytes[i];
        if (!data[i]) fail(SLIDEO_ERR_INVALID_ARG, "page %d is null", i);
        validate_image(w, h, stride);
        GeomEntry& ge = geom_for(m, w, h);
        int cap = std::min(sub_batch_for(m, ge.g, n_pages - i), 64), cnt = 1;
        while (cnt < cap && width[i + cnt] == w && height[i + cnt] == h && stride_bytes[i + cnt] == stride && data[i + cnt]) ++cnt;
        const size_t fb = (size_t)h * stride;
        uint8_t* stage = stage_for_upload(m, S, fb * cnt);
        for (int j = 0; j < cnt; ++j) HIP_CHECK(hipMemcpyAsync(stage + fb * j, data[i + j], fb, hipMemcpyHostToDevice, st));
        const DevFrames staged{stage, w, h, stride, (int64_t)fb};
        const size_t dbytes = m->sift_on ? 128 : 32;                       // descriptor bytes per keypoint
        if (m->sift_on) add_pages_sift(m, S, staged, cnt);                 // -> S.d_kp / S.d_desc / S.orb.qofs, like run_orb
        else run_orb(m, S, staged, cnt, true);
        const uint32_t qtot = S.orb.qtot;
        std::vector<slideo_keypoint> kp(qtot);
        std::vector<uint8_t> desc((size_t)qtot * dbytes);
        if (qtot) {
            HIP_CHECK(hipMemcpyAsync(kp.data(), S.d_kp.p, (size_t)qtot * sizeof(slideo_keypoint), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(desc.data(), S.d_desc.p, (size_t)qtot * dbytes, hipMemcpyDeviceToHost, st));
        }
        int sw = 0, sh = 0;
        run_small(m, staged, cnt, st, &sw, &sh);
        std::vector<uint8_t> smalls((size_t)cnt * sw * sh * 3);
        HIP_CHECK(hipMemcpyAsync(smalls.data(), m->d_small.p, smalls.size(), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const int ac = area_class_for(m, w, h);
        for (int j = 0; j < cnt; ++j) {
            HostPage pg;
            pg.w = w; pg.h = h; pg.sw = sw; pg.sh = sh; pg.area_idx = ac;
            const uint32_t a = S.orb.qofs[j], b = S.orb.qofs[j + 1];
            pg.kp.assign(kp.begin() + a, kp.begin() + b);
            pg.desc.assign(desc.begin() + (size_t)a * dbytes, desc.begin() + (size_t)b * dbytes);
            pg.small_img.assign(smalls.begin() + (size_t)j * sw * sh * 3, smalls.begin() + (size_t)(j + 1) * sw * sh * 3);
            out.push_back(std::move(pg));
            if (m->progress) m->progress(m->progress_user, progress_base + (uint64_t)(i + j + 1), progress_total, "Analyzing PDF pages...");   // lib.rs:49-53
        }
        i += cnt;
    }
}

void append_page(slideo_matcher* m, const HostPage& pg) {
    HostPage c = pg;
    c.area_idx = area_class_for(m, pg.w, pg.h);          // (the size class index is per matcher)
    if (c.sw != m->area_geoms[c.area_idx].dw || c.sh != m->area_geoms[c.area_idx].dh)
        fail(SLIDEO_ERR_INVALID_ARG, "small image %dx%d is not the to_small_image size %dx%d of a %dx%d page", c.sw, c.sh,
             m->area_geoms[c.area_idx].dw, m->area_geoms[c.area_idx].dh, c.w, c.h);
    m->pages.push_back(std::move(c));
}

void set_err(slideo_matcher* m, const char* what) {
    if (m) m->err = what;
    else { std::lock_guard<std::mutex> lk(g_err_mutex); g_create_error = what; }
}

}  // namespace slideo

extern "C" {

uint32_t slideo_abi_version(void) { return SLIDEO_ABI_VERSION; }

void slideo_config_default(slideo_config* c) {
    if (!c) return;
    c->nfeatures = 2000; c->scale_factor = 1.2f; c->nlevels = 8; c->edge_threshold = 62;
    c->patch_size = 62; c->fast_threshold = 20;
    c->knn_k = 30; c->vote_tolerance = 1.05f; c->max_candidate_pages = 40;
    c->ransac_threshold = 3.0; c->ransac_max_iters = 2000; c->ransac_confidence = 0.99; c->refine_iters = 10;
    c->max_rated = 10; c->min_rating = 50.0; c->min_rating_ratio = 0.2;
    c->min_similarity = 0.5f; c->small_area = 300 * 400; c->changed_similarity = 0.98f;
    c->ratio_test = 0.0f;
    c->verify_model = 0;                             // the reference's estimateAffinePartial2D
    c->matcher = 0; c->lsh_tables = 6; c->lsh_key_bits = 12; c->lsh_multi_probe = 1;      // exact search; mo/flann.rs:16-18
    c->verdict_rule = 0;                             // mo/lib.rs:370-389: the best re-projection similarity wins
    std::memset(&c->ocv, 0, sizeof(c->ocv));         // every OpenCV-variant switch at its default
    c->ocv.rng_mul = 4164903690u;                    // CV_RNG_COEFF
    c->ocv.hdlt = 1;                                 // (verify_model 1 only, no reference counterpart: the form proven identical end to end, 1/60 of form 0's cost)
}

const char* slideo_last_error(const slideo_matcher* m) {
    if (m) return m->err.c_str();
    std::lock_guard<std::mutex> lk(g_err_mutex);
    static thread_local std::string copy;
    copy = g_create_error;
    return copy.c_str();
}

// ---- the slots' streams: on hardware queues of their own -------------------------------------------------------------------
// The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) in creation order, and two streams
// on one queue run their kernels one after the other.  The pipeline needs its NSLOTS slot streams to run BESIDE each other (the
// search of one unit over the ORB / verify kernels of the others): when the host has created streams before the matcher — an
// initialised RCCL communicator has — two slot streams would share a queue and the same job runs 10 % slower
// (profiles/r06_experiments.txt 6).  So the streams are picked by measurement: a candidate is kept iff a kernel on it completes
// while spin kernels keep every stream kept so far busy.  ~0.5 ms per candidate at create time; SLIDEO_STREAM_PICK=0: plain
// creation order.  (One 3-line kernel: this unit otherwise holds none.)
__global__ void slideo_spin_kernel(long long ticks) {           // ticks of the 100 MHz wall clock
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
static void pick_independent_streams(hipStream_t* out, int n) {
    using clk = std::chrono::steady_clock;
    std::vector<hipStream_t> rejected;
    int have = 0;
    for (int attempt = 0; have < n && attempt < 4 * n + 8; ++attempt) {
        hipStream_t c = nullptr;
        HIP_CHECK(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
        slideo_spin_kernel<<<1, 64, 0, c>>>(0);                          // (its hardware queue comes into being with its first kernel)
        HIP_CHECK(hipStreamSynchronize(c));
        bool ok = have == 0;
        for (int trial = 0; !ok && trial < 2; ++trial) {                   // (twice: a host thread descheduled for 300 us must not cost a good stream)
            for (int i = 0; i < have; ++i) slideo_spin_kernel<<<1, 64, 0, out[i]>>>(60000);      // 600 us on every stream kept so far
            const auto t0 = clk::now();
            slideo_spin_kernel<<<1, 64, 0, c>>>(0);
            HIP_CHECK(hipStreamSynchronize(c));
            const double us = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
            for (int i = 0; i < have; ++i) HIP_CHECK(hipStreamSynchronize(out[i]));
            ok = us < 300.0;                                               // behind a spinning stream it would have waited the 600
        }
        if (ok) out[have++] = c; else rejected.push_back(c);
    }
    for (; have < n; ++have) {                                             // fewer independent queues than slots (GPU_MAX_HW_QUEUES < NSLOTS): whatever comes
        if (!rejected.empty()) { out[have] = rejected.back(); rejected.pop_back(); }
        else HIP_CHECK(hipStreamCreateWithFlags(&out[have], hipStreamNonBlocking));
    }
    for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
}

int32_t slideo_matcher_create(const slideo_config* cfg, int32_t device, slideo_matcher** out) {
    slideo_matcher* m = nullptr;
    API_TRY
    if (!cfg || !out) fail(SLIDEO_ERR_INVALID_ARG, "null cfg/out");
    *out = nullptr;
    const char* why = "";
    if (!config_supported(*cfg, &why)) fail(SLIDEO_ERR_UNSUPPORTED, "unsupported config: %s", why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(SLIDEO_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) fail(SLIDEO_ERR_INVALID_ARG, "device %d out of range (%d devices)", device, ndev);
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        fail(SLIDEO_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
    HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<slideo_matcher> mm(new slideo_matcher());
    mm->cfg = *cfg; mm->device = device;
    // environment switches of a matcher (include/slideo_amd.h, "Environment"); none changes a result
    { const long v = env_long("SLIDEO_KNN_ENGINE", 0); if (v >= 0 && v <= 3) mm->knn_engine = (int)v; }
    { const long v = env_long("SLIDEO_KNN_SHARE", -1); if ((v >= -1 && v <= 1) || v == 3 || v == 4) mm->knn_share = (int)v; }
    if (const char* e = std::getenv("SLIDEO_KNN_W12_RATIO")) mm->knn_w12_ratio = std::atof(e);
    mm->async_submit = env_long("SLIDEO_ASYNC_SUBMIT", 1) != 0;
    mm->knn_dedup = env_long("SLIDEO_KNN_DEDUP", 1) != 0;
    if (const char* e = std::getenv("SLIDEO_LSH_ENGINE")) mm->lsh_gather = std::string(e) == "gather";
    mm->host_unit = (int)std::max(0l, env_long("SLIDEO_HOST_UNIT", 32));
    mm->orb_chain = env_long("SLIDEO_ORB_CHAIN", 1) != 0;
    {   // a third of a 288 GB device for the SIFT pyramids (a pass of 256 1080p frames: 90 GB; three passes of 86 at 24 GB cost 6 ms of 68);
        // an upper bound only — every call also stays under half of the memory that is free when it runs (stage_sift.hip sift_batch)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b >= ((size_t)192 << 30)) mm->sift_ws_mb = 96l << 10;
    }
    if (const char* e = std::getenv("SLIDEO_WS_GB")) { double gb = std::atof(e); if (gb > 0.1) mm->ws_budget = (size_t)(gb * (double)((size_t)1 << 30)); }
    hipStream_t picked[NSLOTS];
    const bool pick = env_long("SLIDEO_STREAM_PICK", 1) != 0;
    if (pick) pick_independent_streams(picked, NSLOTS);
    int slot_i = 0;
    for (Slot& S : mm->slots) {
        if (pick) S.st = picked[slot_i++];
        else HIP_CHECK(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
        for (auto& e : S.ev) HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipEventCreateWithFlags(&S.ev_in, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&S.ev_orb, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&S.ev_up, hipEventDisableTiming));
    }
    HIP_CHECK(hipStreamCreateWithFlags(&mm->copy_st, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&mm->sift_ev, hipEventDisableTiming));
    mm->stream = mm->slots[0].st;
    orb_stage_init(mm.get());
    {
        // similarity: 2 draws per iteration + redraws; homography: 4 per attempt, several attempts per accepted subset
        int64_t len = std::max<int64_t>(RNG_TABLE_MIN, (cfg->verify_model == 1 ? 64ll : 4ll) * std::max(cfg->ransac_max_iters, 1) + 2048);
        len = std::max<int64_t>(512, env_long("SLIDEO_RNG_STREAM_LEN", (long)len));                        // tests: force the growth path
        upload_rng_stream(mm.get(), (uint32_t)std::min<int64_t>(len, 1ll << 26));
    }
    verify_stage_init(mm.get());
    m = mm.release();
    *out = m;
    API_CATCH(nullptr)
}

#ifdef KT_PROBE
extern "C++" { namespace slideo { void knn_probe_report(); } }
#endif
void slideo_matcher_destroy(slideo_matcher* m) {
#ifdef KT_PROBE
    if (m) { (void)hipDeviceSynchronize(); slideo::knn_probe_report(); }
#endif
    if (!m) return;
    (void)hipSetDevice(m->device);
    for (Slot& S : m->slots) {
        if (S.st) { (void)hipStreamSynchronize(S.st); (void)hipStreamDestroy(S.st); }
        for (auto& e : S.ev) if (e) (void)hipEventDestroy(e);
        if (S.ev_in) (void)hipEventDestroy(S.ev_in);
        if (S.ev_orb) (void)hipEventDestroy(S.ev_orb);
        if (S.ev_up) (void)hipEventDestroy(S.ev_up);
    }
    if (m->copy_st) (void)hipStreamDestroy(m->copy_st);
    if (m->sift_ev) (void)hipEventDestroy(m->sift_ev);
    gate_release(m);
    delete m;
}

int32_t slideo_matcher_max_in_flight(const slideo_matcher* m) { return m ? NSLOTS : 0; }

// ---- working size (include/slideo_amd.h "Working size") ---------------------------------------------------------------------

int32_t slideo_working_size(int32_t w, int32_t h, int32_t max_w, int32_t max_h, int32_t* dw, int32_t* dh) {
    if (w < 1 || h < 1 || max_w < 1 || max_h < 1 || !dw || !dh) return SLIDEO_ERR_INVALID_ARG;
    int a = 0, b = 0;
    working_size_rule(w, h, max_w, max_h, a, b);
    *dw = a; *dh = b;
    return SLIDEO_OK;
}

int32_t slideo_matcher_set_working_size(slideo_matcher* m, int32_t max_w, int32_t max_h) {
    return matcher_set(m, SET_WORKING_SIZE, [&](const FrameSettings& s) { return propose_working_size(s, max_w, max_h); });
}

// ---- frame mask, frame mask scope (include/slideo_amd.h "Frame mask", "Frame mask scope") -----------------------------------

int32_t slideo_matcher_set_frame_mask(slideo_matcher* m, const uint8_t* mask, int32_t width, int32_t height, int32_t stride_bytes) {
    return matcher_set(m, SET_FRAME_MASK, [&](const FrameSettings& s) { return propose_frame_mask(s, mask != nullptr, width, height, stride_bytes); }, mask,
                       stride_bytes);
}

int32_t slideo_matcher_set_frame_mask_scope(slideo_matcher* m, uint32_t scope) {
    return matcher_set(m, SET_FRAME_MASK_SCOPE, [&](const FrameSettings& s) { return propose_frame_mask_scope(s, scope); });
}

int32_t slideo_matcher_frame_mask_scope(const slideo_matcher* m, uint32_t* scope) {
    if (!m || !scope) return SLIDEO_ERR_INVALID_ARG;
    *scope = m->fs.mask_scope;
    return SLIDEO_OK;
}

int32_t slideo_matcher_frame_mask_info(const slideo_matcher* m, int32_t* width, int32_t* height, int32_t* is_set) {
    if (!m || !width || !height || !is_set) return SLIDEO_ERR_INVALID_ARG;
    *width = m->fs.mask.w; *height = m->fs.mask.h; *is_set = m->fs.mask.set ? 1 : 0;
    return SLIDEO_OK;
}

int32_t slideo_matcher_get_working_size(const slideo_matcher* m, int32_t* max_w, int32_t* max_h) {
    if (!m || !max_w || !max_h) return SLIDEO_ERR_INVALID_ARG;
    *max_w = m->fs.work_w; *max_h = m->fs.work_h;
    return SLIDEO_OK;
}

// Tap: one host image reduced to dw x dh (the image a frame of that size stands for when the rule gives dw x dh)
int32_t slideo_reduce_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, int32_t dw, int32_t dh,
                           uint8_t* out, int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !out) fail(SLIDEO_ERR_INVALID_ARG, "null image/out");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    if (width > MAX_DIM || height > MAX_DIM) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", width, height, MAX_DIM);
    if (dw < 1 || dh < 1 || dw > width || dh > height || (dw == width && dh == height))
        fail(SLIDEO_ERR_INVALID_ARG, "reduce %dx%d -> %dx%d: the target must be smaller along at least one side and larger along none", width, height, dw, dh);
    const int64_t ob = (int64_t)dw * dh * 3;
    if (ob > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the reduced image needs %lld bytes", (long long)ob);
    img.plan.unit(PREP_REDUCE, dw, dh, m->cfg.small_area);      // (the tap's own target in place of the working-size rule's)
    tap_staged(m, img, out, ob);
    API_CATCH(m)
}

// ---- frame region (include/slideo_amd.h "Frame region") ---------------------------------------------------------------------

int32_t slideo_matcher_set_frame_region(slideo_matcher* m, int32_t src_w, int32_t src_h, const double* M, int32_t out_w, int32_t out_h) {
    return matcher_set(m, SET_FRAME_REGION, [&](const FrameSettings& s) { return propose_frame_region(s, src_w, src_h, M, out_w, out_h); });
}

int32_t slideo_matcher_frame_region(const slideo_matcher* m, int32_t* src_w, int32_t* src_h, double* M_out, int32_t* out_w, int32_t* out_h,
                                    int32_t* is_set) {
    if (!m || !src_w || !src_h || !M_out || !out_w || !out_h || !is_set) return SLIDEO_ERR_INVALID_ARG;
    const FrameRegion& R = m->fs.region;
    *src_w = R.src_w; *src_h = R.src_h; *out_w = R.out_w; *out_h = R.out_h; *is_set = R.set ? 1 : 0;
    for (int i = 0; i < 9; ++i) M_out[i] = R.M[i];
    return SLIDEO_OK;
}

// the map of a quad (no device, no matcher).  An axis-aligned rectangle in closed form (exact: the crop and the plain scalings);
// any other quad by Gaussian elimination with partial pivoting on the 8x8 system with M8 = 1, in float64
int32_t slideo_frame_region_from_quad(const double* quad, int32_t out_w, int32_t out_h, double* M_out) {
    if (!quad || !M_out || out_w < 2 || out_h < 2 || out_w > MAX_DIM || out_h > MAX_DIM) return SLIDEO_ERR_INVALID_ARG;
    for (int i = 0; i < 8; ++i) if (!std::isfinite(quad[i])) return SLIDEO_ERR_INVALID_ARG;
    // strictly convex, one orientation: the cross products of consecutive edges are nonzero and of one sign
    int pos = 0, neg = 0;
    for (int i = 0; i < 4; ++i) {
        const double* a = quad + 2 * i; const double* b = quad + 2 * ((i + 1) % 4); const double* c = quad + 2 * ((i + 2) % 4);
        const double cr = (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]);
        pos += cr > 0.0; neg += cr < 0.0;
    }
    if (pos != 4 && neg != 4) return SLIDEO_ERR_INVALID_ARG;
    const double U = (double)(out_w - 1), V = (double)(out_h - 1);
    if (quad[0] == quad[6] && quad[2] == quad[4] && quad[1] == quad[3] && quad[5] == quad[7]) {
        const double m[9] = {(quad[2] - quad[0]) / U, 0.0, quad[0], 0.0, (quad[7] - quad[1]) / V, quad[1], 0.0, 0.0, 1.0};
        for (int i = 0; i < 9; ++i) M_out[i] = m[i];
        return SLIDEO_OK;
    }
    const double du[4] = {0.0, U, U, 0.0}, dv[4] = {0.0, 0.0, V, V};
    double A[8][9];
    for (int i = 0; i < 4; ++i) {
        const double x = quad[2 * i], y = quad[2 * i + 1];
        const double r0[9] = {du[i], dv[i], 1.0, 0.0, 0.0, 0.0, -x * du[i], -x * dv[i], x};
        const double r1[9] = {0.0, 0.0, 0.0, du[i], dv[i], 1.0, -y * du[i], -y * dv[i], y};
        for (int j = 0; j < 9; ++j) { A[2 * i][j] = r0[j]; A[2 * i + 1][j] = r1[j]; }
    }
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        for (int r = c + 1; r < 8; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        if (!(std::fabs(A[piv][c]) > 1e-12)) return SLIDEO_ERR_INVALID_ARG;
        if (piv != c) for (int j = 0; j < 9; ++j) std::swap(A[piv][j], A[c][j]);
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int j = c; j < 9; ++j) A[r][j] -= f * A[c][j];
        }
    }
    double sol[8];
    for (int c = 7; c >= 0; --c) {
        double v = A[c][8];
        for (int j = c + 1; j < 8; ++j) v -= A[c][j] * sol[j];
        sol[c] = v / A[c][c];
    }
    for (int i = 0; i < 8; ++i) { if (!std::isfinite(sol[i])) return SLIDEO_ERR_INVALID_ARG; M_out[i] = sol[i]; }
    M_out[8] = 1.0;
    return SLIDEO_OK;
}

// Tap: the rectified image of one host image under the matcher's region (no small_area limit: edge shapes can be small)
int32_t slideo_rectify_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* out,
                            int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !out) fail(SLIDEO_ERR_INVALID_ARG, "null image/out");
    if (!m->fs.region.set) fail(SLIDEO_ERR_STATE, "no frame region is set");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    resolve_unit(m, img, false);                                  // (the tap of the region ALONE: a lens that is set stays out of it)
    const int64_t ob = (int64_t)img.plan.uw * img.plan.uh * 3;
    if (ob > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the rectified image needs %lld bytes", (long long)ob);
    tap_staged(m, img, out, ob);
    API_CATCH(m)
}

// ---- frame lens (include/slideo_amd.h "Frame lens") ---------------------------------------------------------------------------
// The lens commits under the region's row: an idle matcher; it ends the kept frames, the gate state and the match sessions

int32_t slideo_matcher_set_frame_lens(slideo_matcher* m, int32_t src_w, int32_t src_h, double cx, double cy, double f, double k1, double k2) {
    return matcher_set(m, SET_FRAME_REGION, [&](const FrameSettings& s) { return propose_frame_lens(s, src_w, src_h, cx, cy, f, k1, k2); });
}

int32_t slideo_matcher_frame_lens(const slideo_matcher* m, int32_t* src_w, int32_t* src_h, double* cx, double* cy, double* f, double* k1, double* k2,
                                  int32_t* is_set) {
    if (!m || !src_w || !src_h || !cx || !cy || !f || !k1 || !k2 || !is_set) return SLIDEO_ERR_INVALID_ARG;
    const FrameLens& L = m->fs.lens;
    *src_w = L.src_w; *src_h = L.src_h; *cx = L.cx; *cy = L.cy; *f = L.f; *k1 = L.k1; *k2 = L.k2; *is_set = L.set ? 1 : 0;
    return SLIDEO_OK;
}

// step 2 of the definition for one point (no device, no matcher)
int32_t slideo_frame_lens_point(double cx, double cy, double f, double k1, double k2, double u, double v, double* xd, double* yd) {
    if (!xd || !yd) return SLIDEO_ERR_INVALID_ARG;
    const double a[7] = {cx, cy, f, k1, k2, u, v};
    for (double x : a) if (!std::isfinite(x)) return SLIDEO_ERR_INVALID_ARG;
    if (!(f > 0.0)) return SLIDEO_ERR_INVALID_ARG;
    const double q = 1.0 / (f * f);
    if (!std::isfinite(q) || !(q > 0.0)) return SLIDEO_ERR_INVALID_ARG;
    if (k1 == 0.0 && k2 == 0.0) { *xd = u; *yd = v; return SLIDEO_OK; }       // (off: no lens runs, and cx + (u - cx) is not always u)
    frame_lens_point(cx, cy, q, k1, k2, u, v, xd, yd);
    return SLIDEO_OK;
}

// Tap: the analysed image of one host image under the matcher's lens, and its region if one is set (no small_area limit)
int32_t slideo_undistort_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* out,
                              int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !out) fail(SLIDEO_ERR_INVALID_ARG, "null image/out");
    if (!m->fs.lens.set) fail(SLIDEO_ERR_STATE, "no frame lens is set");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    resolve_unit(m, img);
    const int64_t ob = (int64_t)img.plan.uw * img.plan.uh * 3;
    if (ob > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the undistorted image needs %lld bytes", (long long)ob);
    tap_staged(m, img, out, ob);
    API_CATCH(m)
}

int32_t slideo_matcher_set_knn_engine(slideo_matcher* m, int32_t engine) {
    if (!m || engine < 0 || engine > 3) return SLIDEO_ERR_INVALID_ARG;
    m->knn_engine = engine;
    return SLIDEO_OK;
}

int32_t slideo_matcher_set_knn_exact_lists(slideo_matcher* m, int32_t on) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    m->knn_exact_lists = on ? 1 : 0;
    return SLIDEO_OK;
}

int32_t slideo_matcher_set_profiling(slideo_matcher* m, int32_t enable) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    HIP_CHECK(hipSetDevice(m->device));
    m->profiling = enable != 0;
    for (int i = 0; i < SLIDEO_N_STAGES; ++i) { m->prof_ms[i] = 0; m->prof_n[i] = 0; }
    m->prof_pairs = 0;
    m->d_clk.reserve(64);
    HIP_CHECK(hipMemset(m->d_clk.p, 0, 64));
    API_CATCH(m)
}

int32_t slideo_matcher_read_shader_clock(slideo_matcher* m, double* mhz_out, int64_t* samples_out) {
    if (!m || !mhz_out) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    *mhz_out = 0.0;
    if (samples_out) *samples_out = 0;
    if (!m->d_clk.p) return SLIDEO_OK;                       // profiling was never on
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    unsigned long long v[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpy(v, m->d_clk.p, sizeof(v), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemset(m->d_clk.p, 0, 64));
    if (v[1] > 0) *mhz_out = 100.0 * (double)v[0] / (double)v[1];      // s_memrealtime counts 100 MHz
    if (samples_out) *samples_out = (int64_t)v[2];
    API_CATCH(m)
}

int32_t slideo_matcher_read_profile(slideo_matcher* m, double* ms_out, int64_t* launches_out, int64_t* knn_pairs_out) {
    if (!m || !ms_out || !launches_out) return SLIDEO_ERR_INVALID_ARG;
    for (int i = 0; i < SLIDEO_N_STAGES; ++i) { ms_out[i] = m->prof_ms[i]; launches_out[i] = m->prof_n[i]; m->prof_ms[i] = 0; m->prof_n[i] = 0; }
    if (knn_pairs_out) *knn_pairs_out = m->prof_pairs;
    m->prof_pairs = 0;
    return SLIDEO_OK;
}

int32_t slideo_matcher_set_progress(slideo_matcher* m, slideo_progress_fn fn, void* user) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    m->progress = fn; m->progress_user = user;
    return SLIDEO_OK;
}

int32_t slideo_matcher_add_pages_bgr8(slideo_matcher* m, int32_t n_pages, const uint8_t* const* data, const int32_t* width,
                                      const int32_t* height, const int32_t* stride_bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (m->finalized) fail(SLIDEO_ERR_STATE, "pages cannot be added after finalize");
    if (n_pages < 0 || (n_pages > 0 && (!data || !width || !height || !stride_bytes))) fail(SLIDEO_ERR_INVALID_ARG, "null page arrays");
    const uint64_t total = (uint64_t)n_pages;
    if (m->progress) m->progress(m->progress_user, 0, total, "Analyzing PDF pages...");     // lib.rs:43
    std::vector<HostPage> got;
    analyse_pages(m, n_pages, data, width, height, stride_bytes, got, 0, total);
    for (const HostPage& pg : got) append_page(m, pg);
    if (m->progress) m->progress(m->progress_user, total, total, "PDF page analysis successful.");   // lib.rs:58
    API_CATCH(m)
}

int32_t slideo_matcher_add_page_features(slideo_matcher* m, int32_t width, int32_t height, int32_t n_keypoints, const slideo_keypoint* kp,
                                         const uint8_t* desc32, const uint8_t* small_bgr, int32_t small_w, int32_t small_h) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (m->finalized) fail(SLIDEO_ERR_STATE, "pages cannot be added after finalize");
    if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "page features are 32-byte ORB descriptors: not in SIFT mode");
    if (n_keypoints < 0 || (n_keypoints > 0 && (!kp || !desc32)) || !small_bgr) fail(SLIDEO_ERR_INVALID_ARG, "null page feature arrays");
    validate_image(width, height, width * 3);
    HIP_CHECK(hipSetDevice(m->device));
    const int ac = area_class_for(m, width, height);              // (also checks that the page is large enough for to_small_image)
    if (small_w != m->area_geoms[ac].dw || small_h != m->area_geoms[ac].dh)
        fail(SLIDEO_ERR_INVALID_ARG, "small image %dx%d is not the to_small_image size %dx%d of a %dx%d page", small_w, small_h,
             m->area_geoms[ac].dw, m->area_geoms[ac].dh, width, height);
    HostPage pg;
    pg.w = width; pg.h = height; pg.sw = small_w; pg.sh = small_h; pg.area_idx = ac;
    pg.kp.assign(kp, kp + n_keypoints);
    pg.desc.assign(desc32, desc32 + (size_t)n_keypoints * 32);
    pg.small_img.assign(small_bgr, small_bgr + (size_t)small_w * small_h * 3);
    m->pages.push_back(std::move(pg));
    API_CATCH(m)
}

int32_t slideo_matcher_get_page_small(const slideo_matcher* cm, int32_t page_idx, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh) {
    slideo_matcher* m = const_cast<slideo_matcher*>(cm);
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (page_idx < 0 || page_idx >= (int)m->pages.size() || !sw || !sh) fail(SLIDEO_ERR_INVALID_ARG, "page %d out of range", page_idx);
    const HostPage& pg = m->pages[page_idx];
    *sw = pg.sw; *sh = pg.sh;
    if ((int64_t)pg.small_img.size() > out_capacity) fail(SLIDEO_ERR_CAPACITY, "small image needs %zu bytes", pg.small_img.size());
    if (out) std::memcpy(out, pg.small_img.data(), pg.small_img.size());
    API_CATCH(m)
}

int32_t slideo_matcher_finalize_pages(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (m->finalized) fail(SLIDEO_ERR_STATE, "already finalized");
    HIP_CHECK(hipSetDevice(m->device));
    const int P = (int)m->pages.size();
    if (P > 16384) fail(SLIDEO_ERR_UNSUPPORTED, "%d pages exceed the 16384 the vote kernel's LDS layout holds", P);
    int64_t M = 0, small_bytes = 0;
    for (const HostPage& p : m->pages) { M += (int64_t)p.kp.size(); small_bytes += (int64_t)p.small_img.size(); }
    if (M >= ((int64_t)1 << KNN_KEY_SHIFT)) fail(SLIDEO_ERR_UNSUPPORTED, "%lld descriptors exceed 2^23", (long long)M);
    // (the matcher stays open for more pages: the reference's FLANN train on an empty set throws, mo/flann.rs:45-47)
    if (M == 0) fail(SLIDEO_ERR_EMPTY_INDEX, "no page produced a descriptor");
    const size_t dbytes = m->sift_on ? 128 : 32;                           // descriptor bytes per row
    std::vector<uint8_t> train((size_t)M * dbytes);
    std::vector<int32_t> tpage((size_t)M);
    std::vector<float2> xy((size_t)M);
    std::vector<PageInfo> info(P);
    std::vector<uint8_t> smalls((size_t)small_bytes);
    int64_t row = 0, sofs = 0;
    for (int p = 0; p < P; ++p) {
        const HostPage& pg = m->pages[p];
        PageInfo& pi = info[p];
        pi.w = pg.w; pi.h = pg.h; pi.area_idx = pg.area_idx; pi.sw = pg.sw; pi.sh = pg.sh;
        pi.kp_ofs = (int32_t)row; pi.kp_cnt = (int32_t)pg.kp.size(); pi._pad = 0; pi.small_ofs = sofs;
        std::memcpy(train.data() + (size_t)row * dbytes, pg.desc.data(), pg.desc.size());
        for (size_t i = 0; i < pg.kp.size(); ++i) { tpage[row + i] = p; xy[row + i] = make_float2(pg.kp[i].x, pg.kp[i].y); }
        std::memcpy(smalls.data() + sofs, pg.small_img.data(), pg.small_img.size());
        row += (int64_t)pg.kp.size(); sofs += (int64_t)pg.small_img.size();
    }
    m->d_train_page.reserve(std::max<size_t>(tpage.size() * 4, 16));
    m->d_page_xy.reserve(std::max<size_t>(xy.size() * sizeof(float2), 16));
    m->d_pageinfo.reserve(std::max<size_t>(info.size() * sizeof(PageInfo), 16));
    m->d_page_small.reserve(smalls.size() + 16);       // (+ slack: reproject_vt_kernel reads a 3-byte pixel as one dword)
    if (M > 0 && m->sift_on) {
        // SIFT mode: the rows become the train set of the squared-L2 engine (norm order, centred tile-major operand)
        HIP_CHECK(hipMemcpy(m->d_train_page.p, tpage.data(), tpage.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(m->d_page_xy.p, xy.data(), xy.size() * sizeof(float2), hipMemcpyHostToDevice));
        l2_prepare(m->l2, train.data(), (int)M, m->stream);
        m->Mu = M;
    } else if (M > 0) {
        HIP_CHECK(hipMemcpy(m->d_train_page.p, tpage.data(), tpage.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(m->d_page_xy.p, xy.data(), xy.size() * sizeof(float2), hipMemcpyHostToDevice));
        knn_build_index(m, train, M);                  // the Hamming index: distinct rows -> matrix-core operand (+ LSH tables)
    }
    if (P > 0) {
        HIP_CHECK(hipMemcpy(m->d_pageinfo.p, info.data(), info.size() * sizeof(PageInfo), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(m->d_page_small.p, smalls.data(), smalls.size(), hipMemcpyHostToDevice));
    }
    upload_area(m);
    m->M = M;
    m->finalized = true;
    API_CATCH(m)
}

int32_t slideo_matcher_page_count(const slideo_matcher* m) { return m ? (int32_t)m->pages.size() : -1; }
int64_t slideo_matcher_descriptor_count(const slideo_matcher* m) { return m && m->finalized ? m->M : -1; }
int64_t slideo_matcher_unique_descriptor_count(const slideo_matcher* m) { return m && m->finalized ? m->Mu : -1; }

int32_t slideo_matcher_get_page_features(const slideo_matcher* cm, int32_t page_idx, slideo_keypoint* kp, uint8_t* desc32,
                                         int32_t capacity, int32_t* n_out) {
    slideo_matcher* m = const_cast<slideo_matcher*>(cm);
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (page_idx < 0 || page_idx >= (int)m->pages.size()) fail(SLIDEO_ERR_INVALID_ARG, "page %d out of range", page_idx);
    const HostPage& pg = m->pages[page_idx];
    if (n_out) *n_out = (int32_t)pg.kp.size();
    if ((int)pg.kp.size() > capacity) fail(SLIDEO_ERR_CAPACITY, "page has %zu keypoints, capacity %d", pg.kp.size(), capacity);
    if (kp) std::memcpy(kp, pg.kp.data(), pg.kp.size() * sizeof(slideo_keypoint));
    if (desc32) std::memcpy(desc32, pg.desc.data(), pg.desc.size());
    API_CATCH(m)
}

int32_t slideo_match_frames_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                 int32_t stride_bytes, int64_t frame_stride_bytes, slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), verdicts_out, nullptr);
    API_CATCH(m)
}

int32_t slideo_match_frames_bgr8_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                     int32_t stride_bytes, int64_t frame_stride_bytes, slideo_verdict* verdicts_out, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::bgr8(frames_dev, true, width, height, stride_bytes, frame_stride_bytes), verdicts_out,
                      reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_match_frames_submit_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                       int32_t stride_bytes, int64_t frame_stride_bytes, void* hip_stream, int64_t* ticket_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    submit_impl(m, n_frames, FrameSrc::bgr8(frames_dev, true, width, height, stride_bytes, frame_stride_bytes), hip_stream, ticket_out, false);
    API_CATCH(m)
}

int32_t slideo_match_frames_collect_dev(slideo_matcher* m, int64_t ticket, slideo_verdict* verdicts_out, void* verdicts_dev_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!verdicts_out) fail(SLIDEO_ERR_INVALID_ARG, "null verdicts_out");
    HIP_CHECK(hipSetDevice(m->device));
    Slot& S = slot_of_ticket(m, ticket, false);
    unit_collect(m, S, verdicts_out);
    if (verdicts_dev_out) {           // (after the collect: a unit re-run through the exact-size path has rewritten d_verdicts)
        HIP_CHECK(hipMemcpyAsync(verdicts_dev_out, S.d_verdicts.p, (size_t)S.n * sizeof(slideo_verdict), hipMemcpyDeviceToDevice, S.st));
        HIP_CHECK(hipStreamSynchronize(S.st));
    }
    API_CATCH(m)
}

int32_t slideo_match_frames_collect(slideo_matcher* m, int64_t ticket, slideo_verdict* verdicts_out) {
    return slideo_match_frames_collect_dev(m, ticket, verdicts_out, nullptr);
}

int32_t slideo_last_frame_candidates(const slideo_matcher* m, int32_t frame_in_batch, slideo_candidate* out, int32_t capacity,
                                     int32_t* n_out) {
    if (!m || !n_out) return SLIDEO_ERR_INVALID_ARG;
    if (frame_in_batch < 0 || frame_in_batch >= (int)m->last_fcs.size()) return SLIDEO_ERR_INVALID_ARG;
    const FrameCands& fc = m->last_fcs[frame_in_batch];
    *n_out = fc.ncand;
    if (fc.ncand > capacity) return SLIDEO_ERR_CAPACITY;
    for (int i = 0; i < fc.ncand; ++i) {
        slideo_candidate& c = out[i];
        c.page_idx = fc.page[i]; c.n_votes = fc.count[i]; c.inliers = fc.inliers[i]; c.survived = 0; c.similarity = 0.f;
        if (m->cfg.verify_model == 1) { for (int j = 0; j < 9; ++j) c.transform[j] = fc.M[i][j]; }
        else {
            for (int j = 0; j < 6; ++j) c.transform[j] = fc.M[i][j];
            c.transform[6] = c.transform[7] = 0.0; c.transform[8] = fc.found[i] ? 1.0 : 0.0;
        }
        for (int s = 0; s < fc.nsurv; ++s) if (fc.surv[s] == i) { c.survived = 1; c.similarity = fc.sim[s]; }
    }
    return SLIDEO_OK;
}

int32_t slideo_changed_mask_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                 int32_t stride_bytes, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                 uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    changed_mask_impl(m, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), prev_small, last_small_out,
                      changed_out, similarity_out);
    API_CATCH(m)
}

int32_t slideo_match_kept_frames(slideo_matcher* m, int32_t n_sel, const int32_t* sel, slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (n_sel < 0 || (n_sel > 0 && (!sel || !verdicts_out))) fail(SLIDEO_ERR_INVALID_ARG, "null selection/verdicts");
    if (!m->kept.valid) fail(SLIDEO_ERR_STATE, "no frames kept: slideo_changed_mask_bgr8 must be the call before (its upload is what is matched)");
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    const slideo_matcher::Kept k = m->kept;
    const size_t fb = (size_t)k.h * k.stride;
    for (int i = 0; i < n_sel; ++i) if (sel[i] < 0 || sel[i] >= k.n) fail(SLIDEO_ERR_INVALID_ARG, "selected frame %d outside the %d kept", sel[i], k.n);
    if (n_sel == 0) return SLIDEO_OK;
    // the selected frames packed back to back (device to device: 6 MB per 1080p frame at HBM speed), runs of consecutive
    // indices in one copy
    m->d_kept.reserve(fb * (size_t)n_sel + 16);
    hipStream_t st = m->slots[0].st;
    for (int i = 0; i < n_sel;) {
        int j = i + 1;
        while (j < n_sel && sel[j] == sel[j - 1] + 1) ++j;
        HIP_CHECK(hipMemcpyAsync(m->d_kept.as<uint8_t>() + fb * i, m->slots[0].d_stage.as<uint8_t>() + fb * sel[i], fb * (size_t)(j - i), hipMemcpyDeviceToDevice, st));
        i = j;
    }
    FrameSrc kept = FrameSrc::bgr8(m->d_kept.as<uint8_t>(), true, k.w, k.h, k.stride, (int64_t)fb);
    kept.analysed = true;           // (under a frame region the mask call kept the RECTIFIED frames)
    match_frames_impl(m, n_sel, kept, verdicts_out, st);
    API_CATCH(m)
}

// Pins a caller's frame buffer (hipHostRegister) so that the H2D copies of slideo_match_frames_bgr8 / slideo_changed_mask_bgr8
// read it by DMA without the runtime's staging copy.  Worth it for a buffer that is reused across calls (a decoder's frame ring):
// registering costs about as much as one copy of the buffer.
int32_t slideo_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return SLIDEO_ERR_INVALID_ARG;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? SLIDEO_OK : SLIDEO_ERR_HIP;
}
int32_t slideo_host_unregister(void* ptr) {
    if (!ptr) return SLIDEO_ERR_INVALID_ARG;
    return hipHostUnregister(ptr) == hipSuccess ? SLIDEO_OK : SLIDEO_ERR_HIP;
}

// ---- YUV 4:2:0 frames (include/slideo_amd.h "YUV 4:2:0 frames") -------------------------------------------------------------

int32_t slideo_yuv420_layout_packed(int32_t format, int32_t w, int32_t h, slideo_yuv420_layout* out) {
    if (!out || format < SLIDEO_YUV420_NV12 || format > SLIDEO_YUV420_YV12 || w < 1 || h < 1) return SLIDEO_ERR_INVALID_ARG;
    if ((w | h) & 1) return SLIDEO_ERR_UNSUPPORTED;
    const int64_t luma = (int64_t)w * h, chroma = luma / 4;
    slideo_yuv420_layout L{};
    L.y_stride = w;
    if (format == SLIDEO_YUV420_NV12 || format == SLIDEO_YUV420_NV21) {
        L.uv_stride = w; L.uv_step = 2;
        L.u_offset = luma + (format == SLIDEO_YUV420_NV21);
        L.v_offset = luma + (format == SLIDEO_YUV420_NV12);
    } else {
        L.uv_stride = w / 2; L.uv_step = 1;
        L.u_offset = format == SLIDEO_YUV420_I420 ? luma : luma + chroma;
        L.v_offset = format == SLIDEO_YUV420_I420 ? luma + chroma : luma;
    }
    *out = L;
    return SLIDEO_OK;
}

// the same with 16-bit containers: every stride and offset doubled
int32_t slideo_yuv420_layout_packed16(int32_t format, int32_t w, int32_t h, slideo_yuv420_layout* out) {
    slideo_yuv420_layout L{};
    const int32_t rc = slideo_yuv420_layout_packed(format, w, h, out ? &L : nullptr);
    if (rc != SLIDEO_OK) return rc;
    L.y_stride *= 2; L.uv_stride *= 2; L.u_offset *= 2; L.v_offset *= 2;
    *out = L;
    return SLIDEO_OK;
}

// ---- YUV colour description (include/slideo_amd.h "YUV colour description") --------------------------------------------------

int32_t slideo_yuv_coefficients(int32_t matrix, int32_t range, int32_t* out7) {
    if (!out7) return SLIDEO_ERR_INVALID_ARG;
    try { (void)propose_yuv_description(FrameSettings{}, matrix, range, SLIDEO_YUV_DEPTH_8); } catch (const slideo::Error&) { return SLIDEO_ERR_INVALID_ARG; }
    yuv_coefficients(matrix, range, out7);
    return SLIDEO_OK;
}

int32_t slideo_matcher_set_yuv_description(slideo_matcher* m, int32_t matrix, int32_t range, int32_t depth) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_description(s, matrix, range, depth); });
}

int32_t slideo_matcher_yuv_description(const slideo_matcher* m, int32_t* matrix, int32_t* range, int32_t* depth) {
    if (!m || !matrix || !range || !depth) return SLIDEO_ERR_INVALID_ARG;
    *matrix = m->fs.yuv.matrix; *range = m->fs.yuv.range; *depth = m->fs.yuv.depth;
    return SLIDEO_OK;
}

// ---- YUV sampling (include/slideo_amd.h "YUV sampling") -----------------------------------------------------------------------

int32_t slideo_matcher_set_yuv_sampling(slideo_matcher* m, int32_t sampling) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_sampling(s, sampling); });
}

int32_t slideo_matcher_yuv_sampling(const slideo_matcher* m, int32_t* sampling) {
    if (!m || !sampling) return SLIDEO_ERR_INVALID_ARG;
    *sampling = m->fs.yuv.sampling;
    return SLIDEO_OK;
}

// ---- Frame pixel format (include/slideo_amd.h "Frame pixel format") -------------------------------------------------------------

int32_t slideo_matcher_set_pixel_format(slideo_matcher* m, int32_t format) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_pixel_format(s, format); });
}

int32_t slideo_matcher_pixel_format(const slideo_matcher* m, int32_t* format) {
    if (!m || !format) return SLIDEO_ERR_INVALID_ARG;
    *format = m->fs.pixel_format;
    return SLIDEO_OK;
}

int32_t slideo_pixel_format_info(int32_t format, int32_t* bytes_per_pixel, int32_t* planes) {
    int bpp = 0, np = 0;
    if (!pixel_format_info(format, &bpp, &np)) return SLIDEO_ERR_INVALID_ARG;
    if (bytes_per_pixel) *bytes_per_pixel = bpp;
    if (planes) *planes = np;
    return SLIDEO_OK;
}

int32_t slideo_pixels_to_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* bgr_out,
                              int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!frame || !bgr_out) fail(SLIDEO_ERR_INVALID_ARG, "null frame/bgr_out");
    FrameSrc img = FrameSrc::bgr8(frame, false, width, height, stride_bytes, -1);
    img.describe(m->fs);
    img.levels = img.shading = false;               // (the conversion's image: the shading and the levels come behind it, slideo_levels_bgr8)
    validate_frames(img);
    const size_t row = (size_t)width * 3, fb = row * (size_t)height;
    if ((int64_t)fb > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the BGR image needs %zu bytes", fb);
    if (!img.converted()) {                         // the default format: the frame is the image, row by row
        for (int y = 0; y < height; ++y) std::memcpy(bgr_out + (size_t)y * row, frame + (size_t)y * stride_bytes, row);
        return SLIDEO_OK;
    }
    tap_staged(m, img, bgr_out, (int64_t)fb);
    API_CATCH(m)
}

// ---- Frame levels (include/slideo_amd.h "Frame levels"; the learner: stage_activity.hip) -----------------------------------------

int32_t slideo_matcher_set_frame_levels(slideo_matcher* m, const uint8_t* lut768) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_frame_levels(s, lut768, m->levels.on); });
}

int32_t slideo_matcher_frame_levels(const slideo_matcher* m, uint8_t* lut768_out, int32_t* set_out) {
    if (!m || !set_out) return SLIDEO_ERR_INVALID_ARG;
    const FrameLevels& L = m->fs.levels;
    *set_out = L.set ? 1 : 0;
    if (lut768_out)
        for (int i = 0; i < 768; ++i) lut768_out[i] = L.set ? L.lut[i] : (uint8_t)(i & 255);      // (off: the identity)
    return SLIDEO_OK;
}

int32_t slideo_frame_levels_lut(const int32_t* lo, const int32_t* hi, uint8_t* lut768_out) {
    API_TRY
    if (!lo || !hi || !lut768_out) fail(SLIDEO_ERR_INVALID_ARG, "null lo/hi/lut768_out");
    frame_levels_lut(lo, hi, lut768_out);
    API_CATCH(nullptr)
}

// Tap: one host BGR image under the matcher's table, staged and levelled as a frame's unit image is (in place on the slot's stage)
int32_t slideo_levels_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* bgr_out,
                           int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !bgr_out) fail(SLIDEO_ERR_INVALID_ARG, "null bgr/bgr_out");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    img.levels = m->fs.levels.set;                  // (the image is the unit's already: no pixel format, no working size, no region)
    const size_t row = (size_t)width * 3, fb = row * (size_t)height;
    if ((int64_t)fb > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the levelled image needs %zu bytes", fb);
    if (!img.levels) {                              // off: the image itself, row by row
        for (int y = 0; y < height; ++y) std::memcpy(bgr_out + (size_t)y * row, bgr + (size_t)y * stride_bytes, row);
        return SLIDEO_OK;
    }
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    const DevFrames f = stage_frames(m, S, img, 0, 1);
    HIP_CHECK(hipMemcpy2DAsync(bgr_out, row, f.p, (size_t)f.stride, row, (size_t)height, hipMemcpyDeviceToHost, S.st));
    HIP_CHECK(hipStreamSynchronize(S.st));
    API_CATCH(m)
}

// ---- Frame shading (include/slideo_amd.h "Frame shading") ---------------------------------------------------------------------------

int32_t slideo_matcher_set_frame_shading(slideo_matcher* m, int32_t aw, int32_t ah, int32_t cell, const uint16_t* gains) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_frame_shading(s, aw, ah, cell, gains); });
}

int32_t slideo_matcher_frame_shading(const slideo_matcher* m, uint16_t* gains_out, int64_t capacity_elems, int32_t* aw, int32_t* ah, int32_t* cell,
                                     int32_t* set_out) {
    if (!m || !aw || !ah || !cell || !set_out) return SLIDEO_ERR_INVALID_ARG;
    const FrameShading& F = m->fs.shading;
    *set_out = F.set ? 1 : 0;
    *aw = F.aw; *ah = F.ah; *cell = F.cell;
    if (!F.set || !gains_out) return SLIDEO_OK;
    if ((int64_t)F.gains->size() > capacity_elems) return SLIDEO_ERR_CAPACITY;
    std::copy(F.gains->begin(), F.gains->end(), gains_out);
    return SLIDEO_OK;
}

// Tap: one host BGR image of the field's size through shading_kernel as a frame's unit image goes (in place on the slot's stage): the
// plain instance, or with a levels table set the fused one — the shaded and levelled image.  No field: a row-by-row copy
int32_t slideo_shading_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* bgr_out,
                            int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bgr || !bgr_out) fail(SLIDEO_ERR_INVALID_ARG, "null bgr/bgr_out");
    FrameSrc img = FrameSrc::image(bgr, width, height, stride_bytes);
    validate_frames(img);
    img.shading = m->fs.shading.set;                // (the image is the unit's already: no pixel format, no working size, no region)
    img.levels = img.shading && m->fs.levels.set;
    const size_t row = (size_t)width * 3, fb = row * (size_t)height;
    if ((int64_t)fb > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the shaded image needs %zu bytes", fb);
    if (!img.shading) {                             // off: the image itself, row by row
        for (int y = 0; y < height; ++y) std::memcpy(bgr_out + (size_t)y * row, bgr + (size_t)y * stride_bytes, row);
        return SLIDEO_OK;
    }
    if (width != m->fs.shading.aw || height != m->fs.shading.ah)
        fail(SLIDEO_ERR_INVALID_ARG, "a %dx%d image under a frame shading of %dx%d", width, height, m->fs.shading.aw, m->fs.shading.ah);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    const DevFrames f = stage_frames(m, S, img, 0, 1);
    HIP_CHECK(hipMemcpy2DAsync(bgr_out, row, f.p, (size_t)f.stride, row, (size_t)height, hipMemcpyDeviceToHost, S.st));
    HIP_CHECK(hipStreamSynchronize(S.st));
    API_CATCH(m)
}

int32_t slideo_shading_field(const uint64_t* cnt, const uint64_t* sum_f, const uint64_t* sum_p, int32_t gw, int32_t gh, int32_t cell, int64_t min_count,
                             int32_t min_gain_q8, int32_t max_gain_q8, int32_t smooth, uint16_t* gains_out, int32_t* cells_used_out) {
    API_TRY
    if (!shading_field(cnt, sum_f, sum_p, gw, gh, cell, min_count, min_gain_q8, max_gain_q8, smooth, gains_out, cells_used_out))
        return SLIDEO_ERR_INVALID_ARG;
    API_CATCH(nullptr)
}

// ---- YUV chroma filter (include/slideo_amd.h "YUV chroma filter") -------------------------------------------------------------

int32_t slideo_matcher_set_yuv_chroma(slideo_matcher* m, int32_t filter) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_chroma(s, filter); });
}

int32_t slideo_matcher_yuv_chroma(const slideo_matcher* m, int32_t* filter) {
    if (!m || !filter) return SLIDEO_ERR_INVALID_ARG;
    *filter = m->fs.yuv.chroma;
    return SLIDEO_OK;
}

int32_t slideo_yuv_chroma_weights(int32_t filter, int32_t sampling, int32_t* out12) {
    return out12 && yuv_chroma_weights(filter, sampling, out12) ? SLIDEO_OK : SLIDEO_ERR_INVALID_ARG;
}

// ---- YUV transfer (include/slideo_amd.h "YUV transfer") ---------------------------------------------------------------------------

int32_t slideo_matcher_set_yuv_transfer(slideo_matcher* m, int32_t transfer, float white_nits) {
    return matcher_set(m, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_transfer(s, transfer, white_nits); });
}

int32_t slideo_matcher_yuv_transfer(const slideo_matcher* m, int32_t* transfer, float* white_nits) {
    if (!m || !transfer || !white_nits) return SLIDEO_ERR_INVALID_ARG;
    *transfer = m->fs.yuv.transfer; *white_nits = m->fs.yuv.white_nits;
    return SLIDEO_OK;
}

int32_t slideo_yuv_transfer_tables(int32_t transfer, int32_t range, float white_nits, int32_t* coef7, int32_t* gamut9, uint16_t* lin1024,
                                   uint8_t* out4096) {
    return yuv_transfer_tables(transfer, range, white_nits, coef7, gamut9, lin1024, out4096) ? SLIDEO_OK : SLIDEO_ERR_INVALID_ARG;
}

int32_t slideo_yuv_layout_packed(int32_t format, int32_t w, int32_t h, int32_t bytes_per_sample, slideo_yuv420_layout* out) {
    if (!out || format < SLIDEO_YUV422_I422 || format > SLIDEO_YUV444_NV42 || w < 1 || h < 1 || (bytes_per_sample != 1 && bytes_per_sample != 2))
        return SLIDEO_ERR_INVALID_ARG;
    const bool s444 = format >= SLIDEO_YUV444_I444, packed = format >= SLIDEO_YUV422_YUY2 && format <= SLIDEO_YUV422_VYUY;
    if ((!s444 && (w & 1)) || (packed && bytes_per_sample != 1)) return SLIDEO_ERR_UNSUPPORTED;
    const int64_t b = bytes_per_sample;
    slideo_yuv420_layout L{};
    if (packed) {
        L.y_stride = L.uv_stride = 2 * w; L.uv_step = 4;
        L.u_offset = format == SLIDEO_YUV422_YUY2 ? 1 : format == SLIDEO_YUV422_YVYU ? 3 : format == SLIDEO_YUV422_UYVY ? 0 : 2;
        L.v_offset = L.u_offset ^ 2;
        *out = L;
        return SLIDEO_OK;
    }
    const int64_t cw = s444 ? w : w / 2, luma = b * w * h, chroma = b * cw * h;
    const int kind = (format - (s444 ? SLIDEO_YUV444_I444 : SLIDEO_YUV422_I422));      // 0 U V planes, 1 V U planes, 2 U V pairs, 3 V U pairs
    L.y_stride = (int32_t)(b * w);
    if (kind >= 2) {
        L.uv_stride = (int32_t)(2 * b * cw); L.uv_step = 2;
        L.u_offset = luma + (kind == 3 ? b : 0);
        L.v_offset = luma + (kind == 2 ? b : 0);
    } else {
        L.uv_stride = (int32_t)(b * cw); L.uv_step = 1;
        L.u_offset = kind == 0 ? luma : luma + chroma;
        L.v_offset = kind == 0 ? luma + chroma : luma;
    }
    *out = L;
    return SLIDEO_OK;
}

// ---- Frame lists (include/slideo_amd.h "Frame lists"): each form fills a FrameSrc and calls its contiguous twin's driver ------------

int32_t slideo_match_frames_list(slideo_matcher* m, const slideo_frame_list* list, slideo_verdict* verdicts_out, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = FrameSrc::from_list(list, m->fs);
    match_frames_impl(m, list->n_frames, src, verdicts_out, reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

// the submit forms take device lists, as the contiguous submit has no host form
static FrameSrc submit_list_src(slideo_matcher* m, const slideo_frame_list* list) {
    FrameSrc src = FrameSrc::from_list(list, m->fs);
    if (!src.on_device) fail(SLIDEO_ERR_INVALID_ARG, "frame list: a submit form takes device lists (on_device 1); host lists go through the synchronous form");
    return src;
}

int32_t slideo_match_frames_submit_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream, int64_t* ticket_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = submit_list_src(m, list);
    submit_impl(m, list->n_frames, src, hip_stream, ticket_out, false);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_list(slideo_matcher* m, const slideo_frame_list* list, uint8_t* changed_out, float* similarity_out,
                                         slideo_verdict* verdicts_out, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = FrameSrc::from_list(list, m->fs);
    match_frames_impl(m, list->n_frames, src, verdicts_out, reinterpret_cast<hipStream_t>(hip_stream), true, changed_out, similarity_out);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_submit_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream, int64_t* ticket_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = submit_list_src(m, list);
    submit_impl(m, list->n_frames, src, hip_stream, ticket_out, true);
    API_CATCH(m)
}

int32_t slideo_changed_mask_list(slideo_matcher* m, const slideo_frame_list* list, const uint8_t* prev_small, uint8_t* last_small_out,
                                 uint8_t* changed_out, float* similarity_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = FrameSrc::from_list(list, m->fs);
    changed_mask_impl(m, list->n_frames, src, prev_small, last_small_out, changed_out, similarity_out);
    API_CATCH(m)
}

// Tap: the BGR image at source size of every frame of the list (no working size, region or levels), back to back at stride 3 * width
int32_t slideo_frame_list_to_bgr8(slideo_matcher* m, const slideo_frame_list* list, uint8_t* bgr_out, int64_t out_capacity) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    FrameSrc img = FrameSrc::from_list(list, m->fs);
    if (list->n_frames > 0 && !bgr_out) fail(SLIDEO_ERR_INVALID_ARG, "null bgr_out");
    img.describe(m->fs);
    img.levels = img.shading = false;               // (the conversion's image: the shading and the levels come behind it, slideo_levels_bgr8)
    validate_frames(img);
    const int n = list->n_frames;
    const size_t fb = (size_t)list->width * list->height * 3;
    if ((int64_t)(fb * (size_t)n) > out_capacity) fail(SLIDEO_ERR_CAPACITY, "the BGR images need %zu bytes", fb * (size_t)n);
    if (n == 0) return SLIDEO_OK;
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    const int block = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)64 << 20) / fb));
    for (int i = 0; i < n; i += block) {
        const int nb = std::min(block, n - i);
        const DevFrames f = stage_frames(m, S, img, i, nb);
        HIP_CHECK(hipMemcpyAsync(bgr_out + fb * (size_t)i, f.p, fb * (size_t)nb, hipMemcpyDeviceToHost, S.st));
        HIP_CHECK(hipStreamSynchronize(S.st));
    }
    API_CATCH(m)
}

int32_t slideo_match_frames_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                   const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), verdicts_out, nullptr);
    API_CATCH(m)
}

int32_t slideo_match_frames_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                       const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, slideo_verdict* verdicts_out,
                                       void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::yuv420(frames_dev, true, width, height, layout, frame_stride_bytes), verdicts_out,
                      reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_match_frames_submit_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                              const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, void* hip_stream,
                                              int64_t* ticket_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    submit_impl(m, n_frames, FrameSrc::yuv420(frames_dev, true, width, height, layout, frame_stride_bytes), hip_stream, ticket_out, false);
    API_CATCH(m)
}

int32_t slideo_changed_mask_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                   const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                   uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    changed_mask_impl(m, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), prev_small, last_small_out,
                      changed_out, similarity_out);
    API_CATCH(m)
}

// ---- the gated frame calls (include/slideo_amd.h "Changed-frame gate"; the gate itself: stage_gate.hip) ----------------------------

int32_t slideo_match_changed_frames_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height, int32_t stride_bytes,
                                         int64_t frame_stride_bytes, uint8_t* changed_out, float* similarity_out, slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), verdicts_out, nullptr, true,
                      changed_out, similarity_out);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                           const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, uint8_t* changed_out, float* similarity_out,
                                           slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), verdicts_out, nullptr, true,
                      changed_out, similarity_out);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_bgr8_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                             int32_t stride_bytes, int64_t frame_stride_bytes, uint8_t* changed_out, float* similarity_out,
                                             slideo_verdict* verdicts_out, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::bgr8(frames_dev, true, width, height, stride_bytes, frame_stride_bytes), verdicts_out,
                      reinterpret_cast<hipStream_t>(hip_stream), true, changed_out, similarity_out);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                               const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, uint8_t* changed_out,
                                               float* similarity_out, slideo_verdict* verdicts_out, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    match_frames_impl(m, n_frames, FrameSrc::yuv420(frames_dev, true, width, height, layout, frame_stride_bytes), verdicts_out,
                      reinterpret_cast<hipStream_t>(hip_stream), true, changed_out, similarity_out);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_submit_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                               int32_t stride_bytes, int64_t frame_stride_bytes, void* hip_stream, int64_t* ticket_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    submit_impl(m, n_frames, FrameSrc::bgr8(frames_dev, true, width, height, stride_bytes, frame_stride_bytes), hip_stream, ticket_out, true);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_submit_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                                      const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, void* hip_stream,
                                                      int64_t* ticket_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    submit_impl(m, n_frames, FrameSrc::yuv420(frames_dev, true, width, height, layout, frame_stride_bytes), hip_stream, ticket_out, true);
    API_CATCH(m)
}

int32_t slideo_match_changed_frames_collect(slideo_matcher* m, int64_t ticket, uint8_t* changed_out, float* similarity_out, slideo_verdict* verdicts_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!changed_out || !verdicts_out) fail(SLIDEO_ERR_INVALID_ARG, "null changed_out/verdicts_out");
    HIP_CHECK(hipSetDevice(m->device));
    gate_unit_collect(m, slot_of_ticket(m, ticket, true), changed_out, similarity_out, verdicts_out);
    API_CATCH(m)
}

}  // extern "C"
