// stage_activity.hip — the frame activity map of include/slideo_amd.h "Frame activity map": the accumulator's entry points and the
// observe driver (kernels: activity.hip.h).  Observing stages frames as every frame call does (stage_frames) but into a buffer of
// the accumulator's own, and touches nothing else of the matcher: no setting, no gate state, not the frames a mask call kept.
// The observe driver feeds every open accumulator: the activity map's here and, through content_launch (stage_content.hip), the
// content box's (include/slideo_amd.h "Frame content box"), from the same staged block; and the levels histogram's ("Frame levels"),
// whose entry points and kernel (levels.hip.h levels_hist_kernel) live here too.
#include "runtime.hpp"
#include "activity.hip.h"
#define LEVELS_HIST_KERNEL       // (levels_kernel is stage_orb.hip's)
#include "levels.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

namespace {

constexpr int ACT_MAX_BLOCK = 4096;                         // frames per block (the staging kernels' grid.z; sub_batch_for's cap)
static_assert(ACT_MAX_BLOCK <= LVH_MAX_FRAMES, "levels_hist_kernel's u32 bins are bounded by the frames of a block");
constexpr size_t ACT_BLOCK_BYTES = (size_t)256 << 20;       // staging per block of frames (slideo_amd.h states it)

dim3 act_grid(int threads_x, int ah) { return dim3((unsigned)cdiv64(threads_x, ACT_TX), (unsigned)cdiv64(ah, ACT_TY)); }

// slideo_matcher_observe_frames_*: everything is validated before anything is written
void activity_observe(slideo_matcher* m, int n, FrameSrc src, hipStream_t user_stream) {
    if (n < 0 || (n > 0 && !src.p)) fail(SLIDEO_ERR_INVALID_ARG, "null frames");
    src.describe(m->fs);
    validate_frames(src);                                  // a frame source's rules without the deck's (m == nullptr)
    if (!src.converted() && src.frame_stride < (int64_t)src.h * src.stride) fail(SLIDEO_ERR_INVALID_ARG, "frame_stride smaller than one frame");
    resolve_unit(m, src);                                  // the analysed size: the frame region's source-size rule, else the working size
    // the sizes the pipeline analyses, refused as a frame call refuses them: a reduced frame's source (resolve_frames), the unit (geom_for)
    if (src.plan.prep == PREP_REDUCE && (src.w > MAX_DIM || src.h > MAX_DIM)) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", src.w, src.h, MAX_DIM);
    if (src.plan.uw > MAX_DIM || src.plan.uh > MAX_DIM) fail(SLIDEO_ERR_UNSUPPORTED, "image size %dx%d outside 1..%d", src.plan.uw, src.plan.uh, MAX_DIM);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    slideo_matcher::Activity& A = m->activity;
    slideo_matcher::Content& K = m->content;               // (include/slideo_amd.h "Frame content box": the calls feed every open accumulator)
    slideo_matcher::Levels& L = m->levels;                 // (include/slideo_amd.h "Frame levels": likewise; it holds no frame size)
    if (!A.on && !K.on && !L.on) fail(SLIDEO_ERR_STATE, "no activity accumulator: slideo_matcher_activity_begin first");
    if (n == 0) return;
    const int aw = src.plan.uw, ah = src.plan.uh;
    // every check of both accumulators in front of the first write
    if (A.on && A.aw > 0 && (A.aw != aw || A.ah != ah))
        fail(SLIDEO_ERR_STATE, "these frames are analysed at %dx%d, the activity accumulator holds %dx%d: slideo_matcher_activity_begin first", aw, ah,
             A.aw, A.ah);
    if (K.on && K.aw > 0 && (K.aw != aw || K.ah != ah))
        fail(SLIDEO_ERR_STATE, "these frames are analysed at %dx%d, the content accumulator holds %dx%d: slideo_matcher_content_begin first", aw, ah,
             K.aw, K.ah);
    const bool first = A.on && A.aw == 0, kfirst = K.on && K.aw == 0;
    const int64_t pairs = A.pairs + n - (first ? 1 : 0), kframes = K.frames + n;
    if (A.on && pairs > INT32_MAX) fail(SLIDEO_ERR_STATE, "%lld pairs would pass INT32_MAX: read the counts out and begin again", (long long)pairs);
    if (K.on && kframes > INT32_MAX)
        fail(SLIDEO_ERR_STATE, "%lld frames would pass INT32_MAX in the content accumulator: read the counts out and begin again", (long long)kframes);

    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    const size_t px = (size_t)aw * ah;
    // frames per block: what a frame stages in front of its analysed image, and that image unless it is the caller's own memory
    const bool in_place = src.on_device && !src.kernel_in_front();
    const size_t per = src.staging_bytes() + (in_place ? 0 : px * 3);
    const int block = per == 0 ? n : (int)std::min<size_t>({(size_t)n, std::max<size_t>(1, ACT_BLOCK_BYTES / per), (size_t)ACT_MAX_BLOCK});
    // every allocation in front of the first write: the counts and the carried image of a first frame, the largest block's staging
    if (first) { m->d_act_count.reserve(px * 4 + 16); m->d_act_last.reserve(px * 3 + 16); }
    if (kfirst) m->d_cnt_lit.reserve(px * 4 + 16);
    const bool lfirst = L.on && L.frames == 0;
    if (lfirst) m->d_lv_hist.reserve(768 * 8);
    if (!in_place) m->d_act_stage.reserve((size_t)block * px * 3 + 16);
    if (src.on_device && user_stream) {                    // the frames were produced on the caller's stream
        HIP_CHECK(hipEventRecord(S.ev_in, user_stream));
        HIP_CHECK(hipStreamWaitEvent(st, S.ev_in, 0));
    }
    if (first) HIP_CHECK(hipMemsetAsync(m->d_act_count.p, 0, px * 4, st));
    if (kfirst) HIP_CHECK(hipMemsetAsync(m->d_cnt_lit.p, 0, px * 4, st));
    if (lfirst) HIP_CHECK(hipMemsetAsync(m->d_lv_hist.p, 0, 768 * 8, st));
    bool have_prev = A.on && !first;
    try {
        for (int i = 0; i < n; i += block) {
            const int nb = std::min(block, n - i);
            const DevFrames f = stage_frames(m, S, src, i, nb, nullptr, &m->d_act_stage);
            if (f.w != aw || f.h != ah) fail(SLIDEO_ERR_HIP, "internal: staged %dx%d images, the plan says %dx%d", f.w, f.h, aw, ah);
            if (A.on) {
                const ActivityArgs a = activity_args(f.p, f.frame_stride, f.stride, aw, ah, nb, A.delta, have_prev, m->d_act_last.as<uint8_t>(),
                                                     m->d_act_count.as<uint32_t>());
                activity_kernel<<<act_grid((aw + 3) / 4, ah), dim3(ACT_TX, ACT_TY), 0, st>>>(a);
                check_launch("activity_kernel");
                have_prev = true;
            }
            if (K.on) content_launch(m, f, nb, st);        // the same staged frames, directly behind
            if (L.on) {
                const LevelsHistArgs a = levels_hist_args(f.p, f.frame_stride, f.stride, aw, ah, nb, m->d_lv_hist.as<unsigned long long>());
                levels_hist_kernel<<<dim3((unsigned)cdiv64((aw + 3) / 4, LVL_TX), (unsigned)levels_hist_grid_y(ah)), dim3(LVL_TX, LVL_TY), 0, st>>>(a);
                check_launch("levels_hist_kernel");
            }
        }
        HIP_CHECK(hipStreamSynchronize(st));               // (the caller's frames are free again)
    } catch (...) {
        // a device error in the middle of a call: blocks may have been counted that `pairs` and `frames` do not know of.  Both
        // accumulators end (the state "none"): a new begin is needed; so does the levels histogram
        (void)hipStreamSynchronize(st);
        m->activity = slideo_matcher::Activity{};
        m->content = slideo_matcher::Content{};
        m->levels = slideo_matcher::Levels{};
        throw;
    }
    if (A.on) { A.aw = aw; A.ah = ah; A.pairs = pairs; }
    if (K.on) { K.aw = aw; K.ah = ah; K.frames = kframes; }
    if (L.on) { L.frames += n; L.pixels += (int64_t)n * (int64_t)px; }
}

// the histogram of an open session that has observed a frame, on the host
void levels_read(slideo_matcher* m, uint64_t* hist768) {
    require_idle(m);
    if (!m->levels.on || m->levels.frames == 0) fail(SLIDEO_ERR_STATE, "the levels histogram has observed no frame");
    HIP_CHECK(hipSetDevice(m->device));
    HIP_CHECK(hipMemcpyAsync(hist768, m->d_lv_hist.p, 768 * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    const uint64_t px = (uint64_t)m->levels.pixels;
    for (int c = 0; c < 3; ++c) {
        uint64_t t = 0;
        for (int v = 0; v < 256; ++v) t += hist768[c * 256 + v];
        if (t != px) fail(SLIDEO_ERR_HIP, "internal: channel %d of the levels histogram holds %llu samples of %llu", c, (unsigned long long)t, (unsigned long long)px);
    }
}

}  // namespace

}  // namespace slideo

extern "C" {

int32_t slideo_matcher_activity_begin(slideo_matcher* m, int32_t delta) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (delta < 0 || delta > ACT_MAX_DELTA) fail(SLIDEO_ERR_INVALID_ARG, "activity_begin: delta %d outside 0..%d", delta, ACT_MAX_DELTA);
    require_idle(m);
    m->activity = slideo_matcher::Activity{};
    m->activity.on = true; m->activity.delta = delta;
    API_CATCH(m)
}

int32_t slideo_matcher_activity_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    m->activity = slideo_matcher::Activity{};
    m->d_act_count.release(); m->d_act_last.release(); m->d_act_mask.release();
    if (!m->content.on && !m->levels.on) m->d_act_stage.release();      // (shared by the sessions: released when the last of them ends)
    API_CATCH(m)
}

int32_t slideo_matcher_observe_frames_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                           int32_t stride_bytes, int64_t frame_stride_bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    activity_observe(m, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), nullptr);
    API_CATCH(m)
}

int32_t slideo_matcher_observe_frames_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                             const slideo_yuv420_layout* layout, int64_t frame_stride_bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    activity_observe(m, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), nullptr);
    API_CATCH(m)
}

int32_t slideo_matcher_observe_frames_bgr8_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                               int32_t stride_bytes, int64_t frame_stride_bytes, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    activity_observe(m, n_frames, FrameSrc::bgr8(frames_dev, true, width, height, stride_bytes, frame_stride_bytes),
                     reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_matcher_observe_frames_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                                 const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    activity_observe(m, n_frames, FrameSrc::yuv420(frames_dev, true, width, height, layout, frame_stride_bytes),
                     reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_matcher_observe_frames_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = FrameSrc::from_list(list, m->fs);
    activity_observe(m, list->n_frames, src, reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

// ---- the levels histogram (include/slideo_amd.h "Frame levels") -------------------------------------------------------------------

int32_t slideo_matcher_levels_begin(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    if (m->fs.levels.set)
        fail(SLIDEO_ERR_STATE, "levels_begin: a frame levels table is set, and a table learnt on levelled frames is not the source's "
                               "(slideo_matcher_set_frame_levels(m, NULL) first)");
    m->levels = slideo_matcher::Levels{};
    m->levels.on = true;
    API_CATCH(m)
}

int32_t slideo_matcher_levels_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    m->levels = slideo_matcher::Levels{};
    m->d_lv_hist.release();
    if (!m->activity.on && !m->content.on) m->d_act_stage.release();
    API_CATCH(m)
}

int32_t slideo_matcher_levels_info(slideo_matcher* m, int64_t* frames, int64_t* pixels) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!frames || !pixels) fail(SLIDEO_ERR_INVALID_ARG, "null frames/pixels");
    if (!m->levels.on) fail(SLIDEO_ERR_STATE, "no levels histogram: slideo_matcher_levels_begin first");
    *frames = m->levels.frames; *pixels = m->levels.pixels;
    API_CATCH(m)
}

int32_t slideo_matcher_levels_histogram(slideo_matcher* m, uint64_t* hist768) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!hist768) fail(SLIDEO_ERR_INVALID_ARG, "null hist768");
    levels_read(m, hist768);
    API_CATCH(m)
}

int32_t slideo_matcher_levels_points(slideo_matcher* m, int32_t low_ppm, int32_t high_ppm, int32_t* lo3, int32_t* hi3) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!lo3 || !hi3) fail(SLIDEO_ERR_INVALID_ARG, "null lo/hi");
    if (low_ppm < 0 || low_ppm > LEVELS_MAX_PPM || high_ppm < 0 || high_ppm > LEVELS_MAX_PPM)
        fail(SLIDEO_ERR_INVALID_ARG, "levels_points: low_ppm %d, high_ppm %d outside 0..%d", low_ppm, high_ppm, LEVELS_MAX_PPM);
    uint64_t hist[768];
    levels_read(m, hist);
    levels_points(hist, low_ppm, high_ppm, lo3, hi3);
    API_CATCH(m)
}

int32_t slideo_matcher_activity_info(slideo_matcher* m, int32_t* aw, int32_t* ah, int32_t* pairs, int32_t* delta) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!aw || !ah || !pairs || !delta) fail(SLIDEO_ERR_INVALID_ARG, "null aw/ah/pairs/delta");
    const slideo_matcher::Activity& A = m->activity;
    if (!A.on) fail(SLIDEO_ERR_STATE, "no activity accumulator: slideo_matcher_activity_begin first");
    *aw = A.aw; *ah = A.ah; *pairs = (int32_t)A.pairs; *delta = A.delta;
    API_CATCH(m)
}

int32_t slideo_matcher_activity_counts(slideo_matcher* m, uint32_t* out, int64_t capacity_elems, int32_t* aw, int32_t* ah, int32_t* pairs) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!aw || !ah || !pairs) fail(SLIDEO_ERR_INVALID_ARG, "null aw/ah/pairs");
    require_idle(m);
    const slideo_matcher::Activity& A = m->activity;
    if (!A.on || A.aw == 0) fail(SLIDEO_ERR_STATE, "the activity accumulator has observed no frame");
    *aw = A.aw; *ah = A.ah; *pairs = (int32_t)A.pairs;
    if (!out) return SLIDEO_OK;
    const int64_t px = (int64_t)A.aw * A.ah;
    if (px > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the counts need %lld elements", (long long)px);
    HIP_CHECK(hipSetDevice(m->device));
    HIP_CHECK(hipMemcpyAsync(out, m->d_act_count.p, (size_t)px * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    API_CATCH(m)
}

int32_t slideo_matcher_activity_mask(slideo_matcher* m, int32_t max_share_ppm, int32_t grow, uint8_t* out, int64_t capacity, int32_t* aw,
                                     int32_t* ah, int64_t* n_active, int64_t* n_masked) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!out || !aw || !ah || !n_active || !n_masked) fail(SLIDEO_ERR_INVALID_ARG, "null out/aw/ah/n_active/n_masked");
    if (max_share_ppm < 0 || max_share_ppm > ACT_MAX_PPM) fail(SLIDEO_ERR_INVALID_ARG, "activity_mask: max_share_ppm %d outside 0..%d", max_share_ppm, ACT_MAX_PPM);
    if (grow < 0 || grow > ACT_MAX_GROW) fail(SLIDEO_ERR_INVALID_ARG, "activity_mask: grow %d outside 0..%d", grow, ACT_MAX_GROW);
    require_idle(m);
    const slideo_matcher::Activity& A = m->activity;
    if (!A.on || A.pairs == 0) fail(SLIDEO_ERR_STATE, "the activity accumulator holds no pair of frames");
    *aw = A.aw; *ah = A.ah;
    const size_t px = (size_t)A.aw * A.ah;
    if ((int64_t)px > capacity) fail(SLIDEO_ERR_CAPACITY, "the mask needs %lld bytes", (long long)px);
    HIP_CHECK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    // {n_active, n_masked | pass 1 | mask}
    m->d_act_mask.reserve(16 + 2 * px);
    unsigned long long* cnt = m->d_act_mask.as<unsigned long long>();
    ActivityMaskArgs a{};
    a.count = m->d_act_count.as<uint32_t>();
    a.aw = A.aw; a.ah = A.ah; a.grow = grow;
    a.ppm = (uint64_t)max_share_ppm; a.pairs = (uint64_t)A.pairs;
    a.rows = m->d_act_mask.as<uint8_t>() + 16; a.mask = a.rows + px;
    HIP_CHECK(hipMemsetAsync(cnt, 0, 16, st));
    const dim3 grid = act_grid(A.aw, A.ah), blk(ACT_TX, ACT_TY);
    activity_rows_kernel<<<grid, blk, 0, st>>>(a, cnt);
    check_launch("activity_rows_kernel");
    activity_cols_kernel<<<grid, blk, 0, st>>>(a, cnt + 1);
    check_launch("activity_cols_kernel");
    unsigned long long got[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(got, cnt, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(out, a.mask, px, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (got[0] > px || got[1] > px || got[0] > got[1]) fail(SLIDEO_ERR_HIP, "internal: %llu active and %llu masked pixels of %zu", got[0], got[1], px);
    *n_active = (int64_t)got[0]; *n_masked = (int64_t)got[1];
    API_CATCH(m)
}

}  // extern "C"
