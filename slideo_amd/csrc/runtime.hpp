// runtime.hpp — the host runtime behind include/slideo_amd.h, shared by its translation units.
//
//   frame_settings.h   (plain C++) the frame settings record, the setters' range checks, the rules between settings, what a change ends,
//                      the group gate order's rule and the gate state record's header
//   gate_baton.h       (plain C++) the host baton of the group gate chain: publish, fail, await and the guard
//   capi_runtime.hip   handles, page database, slots, the frame settings' one commit path and their set calls, a call's frames resolved
//                      (FrameSrc -> FramePlan) and staged (-> DevFrames), unit submit / collect, the drivers of the frame calls
//                      (pipeline, submit, collect: plain and gated) and their entry points
//   stage_orb.hip      ORB stage drivers          (kernels: orb.hip.h, yuv420.hip.h, yuv_sampling.hip.h, pixel_format.hip.h, reduce.hip.h,
//                                                 frame_region.hip.h, frame_mask.hip.h, levels.hip.h levels_kernel, shading.hip.h, frame_list.hip.h)
//   stage_knn.hip      index build + k-NN stage   (kernels: knn.hip.h, knn_tile.hip.h, knn_l2.hip.h, knn_lsh.hip.h)
//   stage_verify.hip   vote .. verdict, small img (kernels: verify.hip.h, homography.hip.h); the match evidence map's session, its
//                      launch behind the verdicts and its entry points (kernel: evidence.hip.h); the match tone table's likewise (kernel: tone.hip.h),
//                      and the match placement map's (kernel: placement.hip.h)
//   stage_sift.hip     SIFT stage + entry points  (kernels: sift.hip.h)
//   stage_page_set.hip page sets: a subset's search operand built from the finalized deck (kernels: page_set.hip.h)
//   stage_gate.hip     changed-frame gate: gated units, the gate state, its record and its entry points (kernels: gate.hip.h)
//   stage_direct.hip   direct page look-up: the page operand, a gated unit's look-up, its entry points (kernels: direct.hip.h)
//   stage_ssd_table.hip  the SSD-table engine under the direct page look-up and the gate reference ANCHOR: the centred operand, the
//                      table of dot products on the int8 matrix cores, the taps' validity map (kernels: ssd_table.hip.h)
//   stage_activity.hip frame activity map: the accumulator, the observe driver, its entry points (kernels: activity.hip.h); the levels
//                      histogram's session and entry points (kernel: levels.hip.h levels_hist_kernel)
//   stage_content.hip  frame content box: the content accumulator, its launch behind the observe driver, its entry points (kernels: content.hip.h)
//   stage_gate_anchor.hip  gate reference ANCHOR and its gate settle: a gated unit's pair table, carried SSDs, walk and state, the two
//                      settings and the taps (kernels: gate_anchor.hip.h)
//   capi_taps.hip      debug taps of the parity tests
//   capi_group.hip     the N-device group (slideo_group_*), the group gate order and its hand-over from member to member
//
// Every kernel header is compiled by exactly one unit; what crosses units is the functions declared below and the plain
// records of types.h.  There is no CPU fallback anywhere in here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "frame_settings.h"
#include "geom.h"
#include "slideo_amd.h"
#include "types.h"

namespace slideo {

#ifndef SLIDEO_NSLOTS
#define SLIDEO_NSLOTS 4
#endif
constexpr int NSLOTS = SLIDEO_NSLOTS;      // units in flight (each with its own workspace and HIP stream)
constexpr int KLIST = 32;
static_assert(KLIST == VOTE_KLIST, "vote_kernel reads whole key lists");

// Environment switches (all listed in include/slideo_amd.h, "Environment").  None changes a result.
inline long env_long(const char* name, long dflt) {
    const char* e = std::getenv(name);
    return e && *e ? std::atol(e) : dflt;
}

struct GeomEntry {
    int w = 0, h = 0;
    PyrGeom g;
    DevBuf lin_tab;
    DevBuf fast_tiles;                // per FAST tile: level, origin, raw-column alignment (orb.hip.h fast_tile_entry)
};

// One class of the working-size reduce: frames of ag.sw x ag.sh -> ag.dw x ag.dh (reduce.hip.h), with its own tap tables
struct ReduceEntry {
    AreaGeom ag;
    DevBuf d_taps, d_idx;
};

struct HostPage {
    int w = 0, h = 0, sw = 0, sh = 0, area_idx = -1;
    std::vector<slideo_keypoint> kp;
    std::vector<uint8_t> desc;
    std::vector<uint8_t> small_img;
};

// What a call's frames are under the matcher's frame settings: resolved ONCE per call (resolve_frames), read by whatever stages,
// sizes, gates or masks them
enum FramePrep { PREP_NONE, PREP_REDUCE, PREP_RECTIFY };      // the kernel between the BGR view at source size and the unit's image
struct FramePlan {
    FramePrep prep = PREP_NONE;                 // REDUCE: the working size does not hold the frame; RECTIFY: a frame region or lens is set
    bool lens = false;                          // RECTIFY: the launch undistorts under the matcher's frame lens (resolve_unit)
    int uw = 0, uh = 0, sw = 0, sh = 0;         // the BGR image the units read, its small image (small_size under cfg.small_area)
    const uint8_t* mask_pyr = nullptr;          // the frame mask's pyramid for uw x uh (frame_mask_for), null: no filter
    const uint8_t* gate_w = nullptr;            // the gate's validity map for uw x uh (gate_map_for), null: whole small images,
    int npx = 0;                                // and the pixels a similarity is normalised over: the map's n_valid, or sw * sh
    void unit(FramePrep p, int w, int h, int small_area) {
        prep = p; uw = w; uh = h; lens = false;
        small_size(w, h, small_area, sw, sh);
        npx = sw * sh;
    }
};

// A frame list as the library keeps it (include/slideo_amd.h "Frame lists"): its own copy of the addresses, 3 per frame, and the plan
// of its staged layout (frame_settings.h frame_list_plan, whose rules it passed)
struct FrameListData {
    std::vector<const uint8_t*> planes;
    FrameListPlan plan;
};

// A call's frames as the caller handed them over: through the BGR door (yuv null; under the matcher's pixel format) or YUV in the
// layout `yuv`, in host or device memory.
// validate_frames checks them and fills the derived fields; stage_frames turns a block of them into a unit's BGR8 view.
struct FrameSrc {
    const uint8_t* p = nullptr;
    bool on_device = false;
    int w = 0, h = 0;
    int stride = 0;                             // BGR rows; a converted source's BGR image (d_stage) has 3w, set by validate_frames
    int64_t frame_stride = 0;                   // (a single frame: -1 = no stride to check)
    const slideo_yuv420_layout* yuv = nullptr;
    int bps = 1;                                // (derived) bytes per YUV sample: the matcher's YUV description (validate_frames)
    int sampling = SLIDEO_YUV_SAMPLING_420;     // (derived) the matcher's YUV sampling, with bps (describe)
    int chroma = SLIDEO_YUV_CHROMA_NEAREST;     // (derived) the matcher's YUV chroma filter, with them; it changes no byte count
    int64_t yuv_span = 0;                       // (derived) bytes of one YUV frame: its furthest byte + 1
    bool pinned = false;                        // (derived) page-locked host memory: its copies are truly asynchronous DMA
    // the frames are unit images already — the frames a mask call kept (slideo_match_kept_frames): no region applies to them
    bool analysed = false;
    FramePlan plan;                             // (derived) resolve_frames
    // (derived) the matcher's pixel format for frames through the BGR door (describe; YUV and analysed frames: BGR8), the source's
    // row stride and the bytes of one source frame (validate_frames; 0 under BGR8: `stride` is the source's)
    int pixel_format = SLIDEO_PIXEL_BGR8;
    int src_stride = 0;
    int64_t pix_span = 0;
    // (derived) the matcher's frame levels apply: the unit's image goes through the table as the last step (describe; analysed
    // frames are unit images already, levelled when they were kept)
    bool levels = false;
    // (derived) the matcher's frame shading applies: the unit's image is multiplied by the field, in front of the levels (describe;
    // analysed frames were shaded when they were kept)
    bool shading = false;
    // a frame list: the frames are frames list_first .. of `list`, and p, stride, frame_stride and yuv describe the STAGED frames —
    // what stage_frames leaves in the library's memory in front of everything else (p itself: the first frame's first plane)
    std::shared_ptr<const FrameListData> list;
    int list_first = 0;

    void describe(const FrameSettings& fs) {
        bps = fs.yuv.bytes_per_sample(); sampling = fs.yuv.sampling; chroma = fs.yuv.chroma;
        pixel_format = yuv || analysed ? SLIDEO_PIXEL_BGR8 : fs.pixel_format;
        levels = fs.levels.set && !analysed;
        shading = fs.shading.set && !analysed;
    }
    // a converter stands in front of the unit's BGR image: the frames are not read as they lie
    bool converted() const { return yuv != nullptr || pixel_format != SLIDEO_PIXEL_BGR8; }
    int64_t src_span() const { return yuv ? yuv_span : pix_span; }      // bytes of one frame a converter reads
    // a kernel stands in front of the unit's image (a converter, the reduce or the rectify, the shading, the levels): device frames are not the
    // unit's image as they lie in the caller's memory
    // (a list's frames never are: they are gathered first)
    bool kernel_in_front() const { return converted() || plan.prep != PREP_NONE || shading || levels || list; }
    // device frames a converter or a prep kernel reads out of the caller's memory; a list's are staged like a host frame's
    bool in_place() const { return on_device && !list; }

    // per frame, the staging in front of the unit's BGR image: 1.5 B per pixel for 4:2:0 frames, 3 B in 16-bit containers, 2 * bps
    // under both 4:2:2 forms and 3 * bps under 4:4:4 ("YUV sampling"; BGR calls keep their unit sizes); under a pixel format a HOST
    // frame's span (a device frame is converted out of the caller's memory: nothing extra); under frame levels a plain device BGR
    // frame is no longer the caller's own memory below: the table is applied out of it into the unit image (which sub_batch_for
    // counts for every frame) or the gate staging;
    // a reducing or rectifying call: the uploaded source frame (host sources) and the source-sized BGR image of a 4:2:0 frame;
    // gated (a gated call, include/slideo_amd.h "Changed-frame gate"): + the gate staging — the BGR unit image of every frame that
    // is not the caller's own device memory — and the frame's small image (gate_small: at most 3 * small_area bytes) and gate record;
    // a device frame list counts as a host frame does
    size_t staging_bytes(size_t gate_small = 0) const {
        const bool on_device = in_place();
        const size_t px = (size_t)w * h;
        const bool pre = plan.prep != PREP_NONE;
        const size_t yb = (sampling == SLIDEO_YUV_SAMPLING_420 ? px * 3 / 2 : sampling == SLIDEO_YUV_SAMPLING_444 ? px * 3 : px * 2) * (size_t)bps;
        const size_t cb = yuv ? yb : (size_t)pix_span;              // the frame a converter reads (0: plain BGR, no converter)
        size_t b = !pre ? (yuv || !on_device ? cb : 0) : (on_device ? 0 : (converted() ? cb : (size_t)h * stride)) + (converted() ? px * 3 : 0);
        if (gate_small) b += (on_device && !kernel_in_front() ? 0 : (size_t)plan.uw * plan.uh * 3) + gate_small + 32;
        return b;
    }

    static FrameSrc bgr8(const uint8_t* p, bool on_device, int w, int h, int stride, int64_t frame_stride) {
        return FrameSrc{p, on_device, w, h, stride, frame_stride};
    }
    static FrameSrc yuv420(const uint8_t* p, bool on_device, int w, int h, const slideo_yuv420_layout* L, int64_t frame_stride) {
        if (!L) fail(SLIDEO_ERR_INVALID_ARG, "null yuv420 layout");
        FrameSrc s{p, on_device, w, h};
        s.frame_stride = frame_stride; s.yuv = L;
        return s;
    }
    static FrameSrc image(const uint8_t* p, int w, int h, int stride) { return bgr8(p, false, w, h, stride, (int64_t)h * stride); }   // one host image
    // the same frames from frame `first` on (a group member's shard)
    FrameSrc from(int first) const {
        FrameSrc s = *this;
        if (!list) { s.p += (int64_t)first * frame_stride; return s; }
        s.list_first += first;
        s.p = (size_t)s.list_first * 3 < list->planes.size() ? list->planes[(size_t)s.list_first * 3] : nullptr;
        return s;
    }
    // a frame list under the settings fs: every rule of the list checked, the addresses copied (the caller's record and array are
    // free again)
    static FrameSrc from_list(const slideo_frame_list* L, const FrameSettings& fs) {
        auto data = std::make_shared<FrameListData>();
        data->plan = frame_list_plan(L, fs.yuv, fs.pixel_format);
        const uint8_t* const* a = reinterpret_cast<const uint8_t* const*>(L->planes);
        data->planes.assign(a, a + (size_t)L->n_frames * 3);
        const FrameListPlan& P = data->plan;
        FrameSrc s{L->n_frames > 0 ? a[0] : nullptr, L->on_device != 0, L->width, L->height};
        s.frame_stride = P.frame_bytes;
        if (P.yuv_door) s.yuv = &data->plan.yuv; else s.stride = P.stride;
        s.list = std::move(data);
        return s;
    }
    // the plane addresses of list frame `first` of the call (3 per frame)
    const uint8_t* const* list_planes(int first) const { return list->planes.data() + (size_t)(list_first + first) * 3; }
    int list_count() const { return (int)(list->planes.size() / 3) - list_first; }
};

// The BGR8 frames a unit's kernels read (device memory).
struct DevFrames {
    const uint8_t* p = nullptr;
    int w = 0, h = 0, stride = 0;
    int64_t frame_stride = 0;
};

struct OrbOut {            // where the last ORB run of a slot left its results (device)
    uint32_t qtot = 0, max_count = 0;
    int nframes = 0;
    bool full_blur = false;       // stage 1 materialised the whole blurred pyramid (pyramid tap)
    std::vector<uint32_t> qofs;   // host copy, nframes+1
};

// The search of one unit (or tap), as stage_knn.hip knn_plan decides it
struct KnnPlan {
    bool shared = false, w12 = false;   // observed: other units are in flight; the large-deck rule holds (stage_knn.hip knn_plan_unit)
    int nt = 0;                         // train rows searched (unit_collect: the pairs evaluated)
    bool dedup = false;                 // ... which are distinct rows: the keys are expanded along the duplicate chains
    int engine = 0, shape = 0;          // 1 = VALU, 2 / 3 = matrix cores (4 / 2 query tiles per wave); stage_knn.hip KnnShape
    unsigned lds_pad = 0;               // dynamic LDS that keeps the 8-wave block alone on its CU
    int nq_all = 0;                     // the query rows the grid and the buffers cover
    int qblocks = 0, nseg = 0, per_seg = 0;
};

// One workspace + stream.  Several slots let the ORB stage of one unit of frames run concurrently with the
// kNN / verification stages of the previous units (matrix-core bound vs VALU/LDS/HBM bound work).
struct Slot {
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_in = nullptr, ev_orb = nullptr, ev_up = nullptr;
    // arguments of the unit in flight (re-run through the exact-size path if the capacity-sized one overflowed)
    DevFrames u_in; bool u_async = false;
    const uint8_t* u_mask = nullptr;   // the mask pyramid the unit was submitted with (FramePlan::mask_pyr; a re-run filters with it again)
    KnnPlan knn;               // the unit's search as knn_plan_unit decided it (stage_knn.hip)
    int u_set = 0;             // the page set the unit searches (0 = the whole deck), taken from the matcher at submission
    bool u_rerun = false;      // (unit_collect's re-runs: the unit keeps its set)
    DevBuf d_stage, d_pyr, d_blur, d_cand, d_hist, d_candcount, d_flags, d_thr, d_lvlofs, d_kpcount, d_qofs, d_info;
    DevBuf d_items, d_kp, d_desc, d_keys, d_knn_pend, d_votes, d_gpts, d_gmask, d_fcs, d_verdicts, d_pairs, d_blurmask, d_qkeys, d_tail, d_refine;
    DevBuf d_yuv;              // host frames of the unit in front of d_stage: YUV 4:2:0 frames to convert, source-sized frames to reduce
                               // or rectify (reserved by the first YUV, reducing or rectifying call only)
    DevBuf d_ltab;             // a device frame list's plane addresses of the unit (reserved by the first such unit only)
    std::shared_ptr<const FrameListData> u_list;      // ... and the host copy they were uploaded from
    DevBuf d_full;             // the source-sized BGR image of 4:2:0 frames that are reduced or rectified (reserved by the first such call only)
    PinBuf h_info, h_out;
    OrbOut orb;
    // a gated unit (stage_gate.hip): all its frames as BGR unit images (d_gstage; plain device BGR frames stay in the caller's
    // memory), their small images, the gate record {ssd n x u64 | kept idx n x i32 | flags n x u8 | count} and its pinned twin
    DevBuf d_gstage, d_gsmall, d_gate;
    PinBuf h_gate;
    // ... under a direct similarity (stage_direct.hip): the frames' centred operand, {|a'|^2 n x i64 | best n x DirectBest} and the
    // n x np dot products (reserved by the first such unit only)
    DevBuf d_dir_a, d_dir_rec, d_dir_dot;
    // ... under SLIDEO_GATE_ANCHOR (stage_gate_anchor.hip): the frames' centred operand, {|a'|^2 n x i64 | SSDs against the carried
    // anchor n x u64, frame 0 against the carried previous frame u64 | the unit's last anchor i32 | the deferral count behind the
    // unit u32}, and the n x n dot products (reserved by the first such unit only)
    DevBuf d_ga_a, d_ga_rec, d_ga_dot;
    // ... with a gate memory ("Gate memory"): the memory's centred operand, {|e'|^2 64 x i64 | frame 0 against the carried previous
    // frame u64 | the walk's GateMemoryUnit | ref n x i64}, the n x M dot products and the refs' pinned twin (the first such unit only)
    DevBuf d_gm_op, d_gm_rec, d_gm_dot;
    PinBuf h_gm;
    hipEvent_t ev_gate = nullptr;             // the unit's small images are made and the gate state is this unit's last one
    struct GateUnit {
        bool on = false;                      // the unit in flight is gated: slideo_match_changed_frames_collect collects it
        int n = 0, k = 0;                     // frames submitted, frames changed (S.n = k: what the pipeline ran for)
        int sw = 0, sh = 0;
        int npx = 0;                          // the pixels the similarity is normalised over: sw * sh, the gate map's n_valid under one
        bool force0 = false;                  // no gate state at submission: frame 0 is changed, similarity 0.0
        bool settle = false;                  // a gate settle was in force: a frame away from its anchor may be deferred (flag 0)
        bool memory = false;                  // a gate memory was in force: the refs (S.h_gm) tell recalled and deferred frames apart
        int64_t t0 = 0;                       // ... frame 0's ordinal
        // the direct page look-up ran for the unit (direct_t: the matcher's direct similarity at submission): k counts the changed
        // frames that are not direct, the record's tail (direct.hip.h direct_rec_*) is at direct_ofs; has_elig: a page was eligible
        bool direct = false, has_elig = false;
        float direct_t = 0.f;
        size_t direct_ofs = 0;
    } gate;
    // unit in flight
    bool busy = false;
    int64_t ticket = 0;
    int n = 0;
    bool timed = false;

    // Give this (idle) slot the capacities of `o`.  A slot used for the first time would otherwise grow its ~25 buffers
    // (hipFree + hipMalloc, device-wide stalls, tens of ms for the GB-sized ones) in the middle of a steady-state
    // stream of batches; sizing every idle slot when one grows keeps every later unit allocation-free.
    void match_capacity(const Slot& o) {
        // (d_stage is NOT in the list: slot 0's holds the frames slideo_changed_mask_bgr8 kept, and host-frame units size it
        // themselves before their copy)
        DevBuf* mine[] = {&d_pyr, &d_blur, &d_cand, &d_hist, &d_candcount, &d_flags, &d_thr, &d_lvlofs, &d_kpcount, &d_qofs,
                          &d_info, &d_items, &d_kp, &d_desc, &d_keys, &d_knn_pend, &d_votes, &d_gpts, &d_gmask, &d_fcs, &d_verdicts, &d_pairs, &d_blurmask,
                          &d_qkeys, &d_tail, &d_refine};
        const DevBuf* theirs[] = {&o.d_pyr, &o.d_blur, &o.d_cand, &o.d_hist, &o.d_candcount, &o.d_flags, &o.d_thr, &o.d_lvlofs,
                                  &o.d_kpcount, &o.d_qofs, &o.d_info, &o.d_items, &o.d_kp, &o.d_desc, &o.d_keys, &o.d_knn_pend, &o.d_votes,
                                  &o.d_gpts, &o.d_gmask, &o.d_fcs, &o.d_verdicts, &o.d_pairs, &o.d_blurmask, &o.d_qkeys, &o.d_tail, &o.d_refine};
        static_assert(sizeof(mine) / sizeof(mine[0]) == sizeof(theirs) / sizeof(theirs[0]), "same buffer lists");
        for (size_t i = 0; i < sizeof(mine) / sizeof(mine[0]); ++i) mine[i]->reserve_cap(theirs[i]->cap);
        h_info.reserve_cap(o.h_info.cap); h_out.reserve_cap(o.h_out.cap);
    }
};

// The matrix-core search operand of one train set (knn_tile.hip.h): the Hamming deck's, a page set's, the L2 set's, a tap's.  Built
// by stage_knn.hip (prepare_train_bits, l2_prepare) or, a page set's, on the device (stage_page_set.hip).
struct OperandLayout { int st_rows, side_u32; float pad_norm; };   // the side array's shape (knn_tile.hip.h KT_ST_ROWS, KT_SIDE_U32, KT_PAD_NORM)
struct SearchOperand {
    DevBuf tx;                 // [nt_pad][128 B] the rows in stream order, tile-major: {0,1} FP4 (Hamming), centred bytes (L2)
    DevBuf side;               // per super-tile: the rows' norms (Hamming f32, L2 negated i32), then the row ids their keys carry
    DevBuf bound;              // per 32-row tile the bound its first row gives (Hamming: half its norm; L2: its negated norm)
    DevBuf perm;               // [nt_pad] stream row -> source row (-1: a pad row)
    int nt = 0, nt_pad = 0;    // rows, rows padded to whole super-tiles
    size_t bytes() const { return tx.cap + side.cap + bound.cap + perm.cap; }
    // perm_slack: the bytes behind the permutation (the L2 set has never carried them)
    void reserve(int nt_, int nt_pad_, const OperandLayout& L, size_t perm_slack = 16) {
        nt = nt_; nt_pad = nt_pad_;
        tx.reserve((size_t)nt_pad * 128); side.reserve((size_t)(nt_pad / L.st_rows) * L.side_u32 * 4 + 16);
        bound.reserve((size_t)nt_pad / 32 * 4 + 16); perm.reserve((size_t)nt_pad * 4 + perm_slack);
    }
};

// A page set (slideo_matcher_create_page_set): the search operand and duplicate chain of a subset of the finalized deck's pages,
// built on the device (stage_page_set.hip).  Keys carry deck row ids, so everything downstream of the search is the deck's.
struct DirectClass;
struct PageSet {
    int n_pages = 0;
    std::vector<int32_t> pages;                   // the selected deck pages, ascending
    // direct page look-up: per size class of the deck the set's eligible pages, as ascending positions in the class's page list
    // (built on the host at the first gated unit that needs it; the class's operand is the deck's)
    struct DirectElig { const DirectClass* cls = nullptr; int n = 0; DevBuf d; };
    std::vector<std::unique_ptr<DirectElig>> direct_elig;
    int64_t rows = 0, urows = 0;                  // the selected pages' rows, the distinct rows among them (what the search streams)
    SearchOperand op;                             // as prepare_train_bits lays out a deck of exactly the selected pages
    DevBuf d_grp_next;                            // [M] the chain of the selected rows of each duplicate group (-1 elsewhere)
    size_t bytes() const { return op.bytes() + d_grp_next.cap; }
};
constexpr int MAX_PAGE_SETS = 64;                 // live sets per matcher

// Direct page look-up (include/slideo_amd.h "Direct page look-up"): one size class of the deck's small images as the page operand
// of page_ssd_kernel (ssd_table.hip.h: centred i8, MFMA tile order, rows and K padded as ssd_rows_pad and ssd_kp say)
struct DirectClass {
    int sw = 0, sh = 0;
    int np = 0, np_pad = 0;                       // pages of the class, padded to whole wave tiles
    int64_t L = 0, kp = 0;                        // bytes of a small image, padded to the K granule
    std::vector<int32_t> pages;                   // the class's deck pages, ascending
    DevBuf d_op, d_norm, d_pages, d_all;          // operand, |b'|^2 (i64), the page list, the identity eligible list 0 .. np - 1
    // SLIDEO_DIRECT_VALID: |b'|^2 over the valid bytes of the gate's validity map (i64 per page), built at the first look-up under
    // a map of the class's small size and kept while the matcher's fs.gate_map_gen equals norm_v_gen (0: none)
    DevBuf d_norm_v;
    uint64_t norm_v_gen = 0;
};

}  // namespace slideo

struct slideo_matcher {
    slideo_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;      // = slots[0].st (setup, page ingest, taps)
    std::string err;
    slideo_progress_fn progress = nullptr;
    void* progress_user = nullptr;
    size_t ws_budget = (size_t)48 << 30;      // all slots together (SLIDEO_WS_GB); 288 GB of HBM per GPU
    long sift_ws_mb = 24l << 10;              // pyramids of one SIFT pass (SLIDEO_SIFT_WS_MB); 96 GB on a device with >= 192 GB: 256 1080p frames in ONE pass

    slideo::DevBuf d_tables, d_rng, d_ictab;
    struct L2Set { slideo::SearchOperand op; slideo::DevBuf d_keys, d_pend; bool ready = false; } l2;   // cfg2: the L2 train set
    uint32_t rng_len = 0;
    int ic_shift = 0, ic_entries = 0;     // intensity-centroid weight table of describe_kernel (geom.h ic_weight_table)
    std::vector<std::unique_ptr<slideo::GeomEntry>> geoms;
    // the frame settings (changed through settings_commit only) and the device buffers they own: the mask's pyramid, the validity map's weights
    slideo::FrameSettings fs;
    slideo::DevBuf d_mask_pyr, d_gate_w;
    std::vector<std::unique_ptr<slideo::ReduceEntry>> reduces;      // the working-size reduce's size classes

    // INTER_AREA size classes
    std::vector<slideo::AreaGeom> area_geoms;
    std::vector<slideo::AreaTap> area_taps;
    std::vector<int32_t> area_idx;
    std::vector<slideo::AreaRec> area_recs;
    slideo::DevBuf d_area_geoms, d_area_taps, d_area_idx, d_area_recs;
    bool area_dirty = true;

    // pages
    std::vector<slideo::HostPage> pages;
    bool finalized = false;
    // slideo_matcher_use_sift: SIFT features + L2 k-NN + ratio test / tolerance vote in front of the verify stage.  The SIFT and L2
    // workspaces are the matcher's (not a slot's): the extraction stages of consecutive units take turns (sift_ev)
    bool sift_on = false;
    slideo_sift_config sift_cfg{};
    float sift_ratio = 0.f;
    hipEvent_t sift_ev = nullptr;
    bool sift_ev_set = false;
    int64_t M = -1;
    slideo::DevBuf d_train, d_train_page, d_page_xy, d_pageinfo, d_page_small;
    slideo::SearchOperand train_op;    // the deck's {0,1} FP4 operand: its distinct rows in norm order, tiles shuffled (prepare_train_bits)
    // train-set de-duplication (knn.hip.h knn_expand_dups_kernel): the matrix-core engine searches the Mu unique rows, keys carry
    // the lowest original row of a group, d_grp_next chains the equal rows.  SLIDEO_KNN_DEDUP=0 searches all M rows.
    slideo::DevBuf d_utrain, d_grp_next;
    // page sets: what finalize computed on the host for them (the distinct rows' head rows — empty: the identity — and their norm
    // order before the tile shuffle), uploaded by the first slideo_matcher_create_page_set; the live sets by id; the selected one
    std::vector<int32_t> h_urow, h_uorder;
    slideo::DevBuf d_urow, d_uorder;
    std::map<int, std::unique_ptr<slideo::PageSet>> page_sets;
    int cur_set = 0, next_set_id = 1;
    struct LshSet { slideo::DevBuf ofs, rows, keys; slideo::LshDev dev{}; bool ready = false; } lsh;      // slideo_config.matcher 1 (knn_lsh.hip.h)
    int64_t Mu = -1;
    int knn_dedup = 1;
    int lsh_gather = 0;              // SLIDEO_LSH_ENGINE=gather: matcher 1 through knn_lsh_kernel (buckets gathered) instead of the filtered matrix-core stream
    int host_unit = 32;              // frames per unit of a HOST-memory batch (SLIDEO_HOST_UNIT; 0 = the device-path rule)
    // every H2D copy of frame units goes through ONE stream, in submission order: copies issued on the units' own streams run
    // concurrently and share the link, so the first unit's frames arrive when all of them have (measured: 39 - 45 ms per 256
    // frames from pinned memory against 31 in order)
    hipStream_t copy_st = nullptr;
    // the frames slideo_changed_mask_bgr8 uploaded last (slot 0's staging buffer), for slideo_match_kept_frames
    struct Kept { bool valid = false; int n = 0, w = 0, h = 0, stride = 0; } kept;
    slideo::DevBuf d_kept;
    bool units_pending = false;   // the call being served has more units than the one submitted now
    double knn_w12_ratio = 290.0;   // the large-deck rule of the search's block shape (stage_knn.hip knn_plan_unit; SLIDEO_KNN_W12_RATIO)
    int knn_share = -1;     // the search's block shape (SLIDEO_KNN_SHARE; stage_knn.hip knn_shape): -1 = while other units are in flight one 8-wave block per CU,
                            // or the 12-wave block for large decks (knn_w12_ratio), two 8-wave blocks otherwise (default); 0 = always two 8-wave blocks;
                            // 1 = always one; 3 / 4 = the 12-wave block while shared / always
    int knn_engine = 0;     // 0 = FP4 MFMA, wave shape chosen per launch (default), 1 = integer VALU popcount,
                            // 2 = FP4 MFMA, 2 waves/SIMD x 4 query tiles (knn_tile4_kernel), 3 = 4 waves/SIMD x 2 tiles (knn_tile2_kernel)
    int knn_exact_lists = 0;  // 1 = the matcher's kNN stage keeps full exact k-NN lists (no fused vote filter)
    // Units are enqueued in one go, without the mid-unit host wait for the keypoint counts: everything downstream of the ORB
    // counts is sized by capacity and reads the counts on the device (SLIDEO_ASYNC_SUBMIT=0: the exact-size path with the wait).
    int async_submit = 1;
    // ORB stages of consecutive units take turns (each waits for the previous unit's ORB stage on the GPU, event to event):
    // what the host wait used to enforce as a side effect (SLIDEO_ORB_CHAIN=0: free-running).
    int orb_chain = 1;
    hipEvent_t last_orb_ev = nullptr;

    // changed-frame gate (include/slideo_amd.h "Changed-frame gate"): the small image of the last gated frame (device), and what
    // the gated frames since the last reset were.  A gated unit's pair-0 SSD and its write of the new state wait for the previous
    // gated unit's (last_gate_ev, event to event, as last_orb_ev chains the ORB stages).
    struct GateState {
        bool has = false;                     // false: "none", the next gated frame is changed
        bool seen = false;                    // frames were gated since the reset: w, h, yuv are theirs
        int w = 0, h = 0; bool yuv = false;
        int sw = 0, sh = 0;                   // (has) the small image's size
        int64_t next_ord = 0;                 // the next gated frame's ordinal ("Gate memory"): frames gated since the last reset
    } gate;
    slideo::DevBuf d_gate_small;
    // under a gate settle (include/slideo_amd.h "Gate settle") d_gate_small is the anchor's; beside it the small image of the
    // previous gated frame and the deferral count (u32), written and read where d_gate_small is
    slideo::DevBuf d_gate_prev, d_gate_d;
    hipEvent_t last_gate_ev = nullptr;
    // gate memory (include/slideo_amd.h "Gate memory"), while fs.gate_memory = M > 0: the M small images of the ring (gm_stride
    // bytes apart) and its GateMemoryMeta; d_gate_small is then written by the resets alone and d_gate_d not at all (d is the
    // meta's).  gate_refs: the refs of the last synchronous gated call or the last collected gated ticket (gate_refs_valid: there
    // was one since the setting; gate_refs_call: a synchronous call is appending its units')
    slideo::DevBuf d_gm_img, d_gm_meta;
    int64_t gm_stride = 0;
    std::vector<int64_t> gate_refs;
    bool gate_refs_valid = false, gate_refs_call = false;
    // group gate chain (include/slideo_amd.h "Group gate order"; capi_group.hip sets both for ONE gated call, a single matcher never).
    // gate_receive: called once, on the first gated unit's stream, exactly where that unit waits for the previous gated unit's write of
    // the state — it blocks the host until the predecessor's state has arrived and queues its copy into the three state buffers.
    // gate_publish: called once behind the submission of the call's last unit, whose ev_gate marks the state the successor receives.
    std::function<void(hipStream_t)> gate_receive;
    std::function<void(slideo::Slot&)> gate_publish;

    // frame activity map (include/slideo_amd.h "Frame activity map"): the accumulator — "none" (on false), empty (aw 0) or the counts
    // of `pairs` consecutive pairs of aw x ah analysed images — and its device buffers: the counts (u32), the carried last image, the
    // staging of a block of observed frames (stage_frames' `into`) and the read-out's {counters | pass 1 | mask}
    struct Activity { bool on = false; int aw = 0, ah = 0, delta = 0; int64_t pairs = 0; } activity;
    slideo::DevBuf d_act_count, d_act_last, d_act_stage, d_act_mask;

    // frame content box (include/slideo_amd.h "Frame content box"): the content accumulator — "none" (on false), empty (aw 0) or the
    // lit counts of `frames` aw x ah analysed images — and its device buffers: the counts (u32) and the read-out's {n_content | row
    // fills | column fills}.  The observe calls feed it beside the activity accumulator, from the same staged block (d_act_stage,
    // released when the last of the two ends)
    struct Content { bool on = false; int aw = 0, ah = 0, level = 0; int64_t frames = 0; } content;
    slideo::DevBuf d_cnt_lit, d_cnt_fill;

    // frame levels (include/slideo_amd.h "Frame levels"): the device copy of fs.levels.lut (written by settings_commit while the
    // matcher is idle), and the levels histogram — "none" (on false) or the per-channel counts (u64 [3][256], d_lv_hist) of `frames`
    // analysed images of `pixels` pixels in all, of any sizes.  The observe calls feed it beside the other two accumulators
    slideo::DevBuf d_levels;
    // frame shading (include/slideo_amd.h "Frame shading"): the device copy of fs.shading.gains (u16 [gh + 1][gw + 1]), written by
    // settings_commit while the matcher is idle
    slideo::DevBuf d_shading;
    // YUV transfer (include/slideo_amd.h "YUV transfer"): the device copy of LIN (uint16 [1024]) and OUT (uint8 [4096]) of
    // (fs.yuv.transfer, fs.yuv.white_nits), 6144 bytes, rewritten by settings_commit while the matcher is idle
    slideo::DevBuf d_transfer;
    struct Levels { bool on = false; int64_t frames = 0, pixels = 0; } levels;
    slideo::DevBuf d_lv_hist;

    // match evidence map (include/slideo_amd.h "Match evidence map"): the session — "none" (on false), empty (aw 0) or the counts of
    // the match calls since evidence_begin at the analysed size aw x ah — and its device buffer {seen [gh][gw] | hit [gh][gw]} (u32),
    // which evidence_kernel adds to on the units' streams.  through, counted: the frames of the collected units (unit_collect)
    // max_frames: the session's frames limit, 2^20 unless SLIDEO_EVIDENCE_MAX_FRAMES lowered it at begin (the tests' seam)
    struct Evidence { bool on = false; int cell = 0, min_inliers = 0, aw = 0, ah = 0, gw = 0, gh = 0; int64_t through = 0, counted = 0, max_frames = 0; } evidence;
    slideo::DevBuf d_evidence;

    // match tone table (include/slideo_amd.h "Match tone table"): the session — "none" (on false) or the settings of tone_begin and the
    // frames of the collected units (through) — and its device buffer {cnt u64 [3][256] | sum u64 [3][256] | frames_counted u64},
    // zeroed at begin, which tone_kernel adds to on the units' streams.  max_frames: 2^31 unless SLIDEO_TONE_MAX_FRAMES lowered it at begin
    struct Tone { bool on = false; int min_inliers = 0, min_hits = 0, flat = 0; int64_t through = 0, max_frames = 0; } tone;
    slideo::DevBuf d_tone;

    // match placement map (include/slideo_amd.h "Match placement map"): the session — "none" (on false), empty (aw 0) or the sums of
    // the match calls since placement_begin at the analysed size aw x ah — and its device buffer {n | sfx | sfy | su | sv} (u64
    // [gh][gw] each) | frames_counted u64, zeroed at the first counted call, which placement_kernel adds to on the units' streams.
    // through: the frames of the collected units.  max_frames: 2^20 unless SLIDEO_PLACEMENT_MAX_FRAMES lowered it at begin
    struct Placement { bool on = false; int cell = 0, min_inliers = 0, aw = 0, ah = 0, gw = 0, gh = 0; double reach = 0; int64_t through = 0, max_frames = 0; } placement;
    slideo::DevBuf d_placement;

    // match shading map (include/slideo_amd.h "Match shading map"): the session — "none" (on false), empty (aw 0) or the sums of the
    // match calls since shading_begin at the analysed size aw x ah — and its device buffer {cnt | sum_f | sum_p} (u64 [gh][gw] each)
    // | frames_counted u64, zeroed at the first counted call, which shading_map_kernel adds to on the units' streams.  through: the
    // frames of the collected units.  max_frames: 2^20 unless SLIDEO_SHADING_MAX_FRAMES lowered it at begin
    struct ShadingMap { bool on = false; int cell = 0, min_inliers = 0, min_hits = 0, flat = 0, aw = 0, ah = 0, gw = 0, gh = 0; int64_t through = 0, max_frames = 0; } shading_map;
    slideo::DevBuf d_shading_map;

    // direct page look-up (include/slideo_amd.h "Direct page look-up"): built at the first use with fs.direct_t > 0 after finalize, the
    // deck's size classes
    bool direct_built = false;
    std::vector<std::unique_ptr<slideo::DirectClass>> direct_classes;

    // workspaces
    slideo::Slot slots[slideo::NSLOTS];
    int next_slot = 0;
    int64_t next_ticket = 1;
    slideo::DevBuf d_small, d_ssd, d_prev_small, d_tapq, d_tapt, d_tapidx, d_tapdist;
    struct SiftWs { slideo::DevBuf base, gauss, gray, cand, counts, raw, items, kept, qofs, info, kp, desc; } sift;     // csrc/sift.hip.h

    // stage profiling (HIP events on the launch streams)
    bool profiling = false;
    double prof_ms[SLIDEO_N_STAGES] = {0, 0, 0, 0};
    int64_t prof_n[SLIDEO_N_STAGES] = {0, 0, 0, 0};
    int64_t prof_pairs = 0;
    slideo::DevBuf d_clk;           // {shader cycles, 100 MHz ticks, samples} summed by the search blocks while profiling (knn_tile.hip.h KtClock)

    // trace of the last match call
    std::vector<slideo::FrameCands> last_fcs;
};

namespace slideo {

// ---- capi_runtime.hip ---------------------------------------------------------------------------
void set_err(slideo_matcher* m, const char* what);
void check_launch(const char* what);
GeomEntry& geom_for(slideo_matcher* m, int w, int h);
int area_class_for(slideo_matcher* m, int w, int h);
void upload_area(slideo_matcher* m);
inline bool blur_is_f32(const slideo_matcher* m) { return m->cfg.ocv.blur <= 1; }
uint32_t kp_cap_for(const slideo_matcher* m, const PyrGeom& g);
// staging: bytes per frame in front of the unit's BGR image (FrameSrc::staging_bytes)
// fixed: bytes a unit takes whatever its frame count (gate_memory_budget), taken out of the slot's share before the frames are counted
int sub_batch_for(slideo_matcher* m, const PyrGeom& g, int n, size_t staging = 0, size_t fixed = 0);
void require_idle(slideo_matcher* m);
void validate_image(int w, int h, int stride);
// The argument rules of a call's frames (include/slideo_amd.h), in the order the entry points report them: a YUV source's layout
// (its span; the stride of its BGR image), then — m != null: a match call — the matcher's state and the null frames / verdicts
// `out`, then a BGR source's geometry, what resolve_frames reports and — match calls — a BGR source's frame stride.
void validate_frames(FrameSrc& src, slideo_matcher* m = nullptr, int n = 0, const void* out = nullptr);
// The resolver of src.plan from m's frame settings and a validated source, in this order: prep, unit and small size — the frame
// region (SLIDEO_ERR_INVALID_ARG at another size than its source; none for analysed frames), else the working size —; match: the source
// limit of a reduced frame, the SIFT limits, the page set's modes, the mask's pyramid (frame_mask_for); the gate's weights and npx.
void resolve_frames(const slideo_matcher* m, FrameSrc& src, bool match);
// its first step alone: prep, unit size and small size of a validated source (what an observe call needs: no mask, no gate map)
// with_lens false: the frame lens stays out of it (slideo_rectify_bgr8, the tap of the region alone); else a lens that is set makes
// the call a rectifying one of the region's output size, or of the lens's source size where no region is set
void resolve_unit(const slideo_matcher* m, FrameSrc& src, bool with_lens = true);
// The one path by which a frame setting of m changes: idle (SLIDEO_ERR_STATE), the rules between settings on `next` (a propose_*
// of frame_settings.h), what the mask and its scope need on the device built first and installed on success (mask: the host mask
// of SET_FRAME_MASK, rows `stride` apart), then `next` in force and what SETTING_ENDS[what] ends ended.
void settings_commit(slideo_matcher* m, Setting what, FrameSettings next, const uint8_t* mask = nullptr, int stride = 0);
// Frames [first, first + n) of a validated `src` as BGR8 on the device, for slot S: a device BGR source as it is; host frames
// copied into S.d_stage (BGR) or S.d_yuv (YUV, another pixel format), on `cs` when given (S.st waits for it) and on S.st otherwise; YUV and other pixel formats converted into
// S.d_stage on S.st (device frames of another pixel format out of the caller's memory); a source the working size reduces: host frames into S.d_yuv, 4:2:0 frames converted into S.d_full, then
// reduced into S.d_stage; under a frame region the same with the rectify in place of the reduce (device BGR frames are read in the
// caller's memory); the DevFrames are then plan.uw x plan.uh.  Every write of a slot's d_stage goes through here (page ingest through its staging buffer) and ends the
// frames slideo_changed_mask_bgr8 kept for slideo_match_kept_frames.  Under frame levels (src.levels) the table is applied last, in
// place on what was staged; a plain device BGR source, otherwise returned as it is, is levelled out of the caller's memory into the stage.
// into: the staging buffer in place of S.d_stage (a gated unit's S.d_gstage; the kept frames of a mask call then stay).
DevFrames stage_frames(slideo_matcher* m, Slot& S, const FrameSrc& src, int first, int n, hipStream_t cs = nullptr, DevBuf* into = nullptr);
// stage_content.hip: content_kernel over a staged block of n frames into m's content accumulator (m->content.on; d_cnt_lit holds
// f.w x f.h counts), on `st`.  Called by the observe driver (stage_activity.hip) behind or in place of activity_kernel.
void content_launch(slideo_matcher* m, const DevFrames& f, int n, hipStream_t st);
void upload_rng_stream(slideo_matcher* m, uint32_t len);
// mask_pyr: the frame mask pyramid of the unit (FramePlan::mask_pyr), kept in S.u_mask
void unit_submit(slideo_matcher* m, Slot& S, const DevFrames& f, int n, const uint8_t* mask_pyr, bool allow_async = true);
void unit_collect(slideo_matcher* m, Slot& S, slideo_verdict* out_host);
// a synchronous frame call through the unit pipeline; gated: through the gate (changed_out, similarity_out as the gated entry points')
void match_frames_impl(slideo_matcher* m, int n, FrameSrc src, slideo_verdict* out, hipStream_t user_stream, bool gated = false,
                       uint8_t* changed_out = nullptr, float* similarity_out = nullptr);
// slideo_changed_mask_bgr8 / _yuv420: the frames stay in slot 0's d_stage, which m->kept then describes
void changed_mask_impl(slideo_matcher* m, int n, FrameSrc src, const uint8_t* prev_small, uint8_t* last_small_out, uint8_t* changed_out,
                       float* similarity_out);
// the similarity MarkSimilarIter compares (video_capture.rs:86-98) from the integer SSD of two sw x sh small images: the ONE host
// expression behind the mask calls' flags, the gate's similarities and slideo_changed_ssd_threshold
// (n pixels: sw * sh, or the n_valid of the frame mask's GATE scope)
inline float changed_similarity(unsigned long long ssd, int n) {
    double e = std::sqrt((double)ssd);
    float max_error = std::sqrt((255.0f * 255.0f * 3.0f) * (float)n);
    return 1.0f - (float)e / max_error;
}
// S's staging buffer with room for `bytes` (ends the kept frames of a mask call)
uint8_t* stage_for_upload(slideo_matcher* m, Slot& S, size_t bytes);
// the image taps: the one image of `img` staged on slot 0 (idle matcher), its ob bytes to the host
void tap_staged(slideo_matcher* m, const FrameSrc& img, uint8_t* out, int64_t ob);
// ProcessedImage::compute over n host pages (mo/lib.rs:92-131) WITHOUT appending them: the analysed pages, in order, into `out`
void analyse_pages(slideo_matcher* m, int n_pages, const uint8_t* const* data, const int32_t* width, const int32_t* height, const int32_t* stride_bytes,
                   std::vector<HostPage>& out, uint64_t progress_base, uint64_t progress_total);
// appends an analysed page (this matcher's own, or another device's of the same config: the records are plain host data)
void append_page(slideo_matcher* m, const HostPage& pg);

// ---- stage_orb.hip --------------------------------------------------------------------------------
void orb_stage_init(slideo_matcher* m);          // device tables of the ORB kernels + their launch attributes (slideo_matcher_create)
void orb_geom_init(slideo_matcher* m, GeomEntry& e, const std::vector<uint32_t>& lin_tab);      // per frame size: the kernels' device tables
// mask_pyr: the mask pyramid of frames of f's size (frame_mask_for), nullptr: no mask — pages, and frames of a matcher without one
void orb_stage1(slideo_matcher* m, Slot& S, const DevFrames& f, int n, bool with_blur = false, uint32_t kp_cap = 0xFFFFFFFFu,
                const uint8_t* mask_pyr = nullptr);
void orb_wait_info(slideo_matcher* m, Slot& S);
void orb_stage2(slideo_matcher* m, Slot& S, int w, int h, bool by_capacity = false);
void run_orb(slideo_matcher* m, Slot& S, const DevFrames& f, int n, bool keep_host_qofs, bool with_blur = false, const uint8_t* mask_pyr = nullptr);
// Frame mask (include/slideo_amd.h "Frame mask").  frame_mask_build: the pyramid of the w x h mask (rows `stride` apart, host memory)
// into `out` on m->stream (settings_commit installs it).  frame_mask_for: the pyramid a frame call of analysed size w x h
// filters its candidates with — nullptr without a mask, SLIDEO_ERR_INVALID_ARG at another size.
void frame_mask_build(slideo_matcher* m, const uint8_t* mask, int w, int h, int stride, DevBuf& out);
const uint8_t* frame_mask_for(const slideo_matcher* m, int w, int h);
// the two ORB kernels the SIFT stage shares: BGR -> gray u8 (pitch `pitch`, frame stride gframe), and the per-frame offsets scan
void orb_launch_gray(const slideo_matcher* m, const uint8_t* frames_dev, int64_t frame_stride, int stride, uint8_t* gray, int64_t gframe, int w, int h,
                     int pitch, int n, hipStream_t st);
void orb_launch_scan(const uint32_t* counts, int n, uint32_t* qofs, uint32_t* info, hipStream_t st);
// n BGR8 frames of w x h -> cv::resize(INTER_AREA) to dw x dh under m's ocv.area, at dst (stride 3dw, frame stride 3dw dh)
void launch_reduce(slideo_matcher* m, const uint8_t* src, int64_t src_fs, int stride, int w, int h, int dw, int dh, int n, uint8_t* dst,
                   hipStream_t st);
// n BGR8 frames of R.src_w x R.src_h -> their rectified R.out_w x R.out_h images at dst (stride 3 out_w, frame stride 3 out_w out_h)
// L: the lens that is set, undistorted in the same launch (frame_lens.hip.h; without a region: at the lens's source size); null: none
void launch_rectify(const FrameRegion& R, const FrameLens* L, const uint8_t* src, int64_t src_fs, int stride, int n, uint8_t* dst, hipStream_t st);
// step 2 of "Frame lens" for one point, the kernel's own host build (q = 1.0 / (f * f))
void frame_lens_point(double cx, double cy, double q, double k1, double k2, double u, double v, double* xd, double* yd);
// the rectify_kernel instance of a map: R.kind, R.tx, R.ty from R.M
void frame_region_classify(FrameRegion& R);
// n decoded YUV 4:2:0 frames (a layout yuv420_validate accepted under `desc`, frame stride src_fs) -> BGR8 at dst, stride 3w, frame
// stride 3wh.  One kernel family per call (stage_orb.hip): transfer, chroma filter, sampling, else yuv420_to_bgr_desc_kernel.  transfer_tab: the matcher's
// d_transfer, read under a transfer other than SDR alone (yuv_transfer_to_bgr_kernel)
void launch_yuv420_to_bgr(const YuvDesc& desc, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h, int n, uint8_t* dst, hipStream_t st,
                          const uint32_t* transfer_tab = nullptr);
// n frames under the pixel format `format` (not SLIDEO_PIXEL_BGR8; a layout pixel_format_validate accepted, rows `stride` and frames
// src_fs apart) -> BGR8 at dst, stride 3w, frame stride 3wh: pixels_to_bgr_kernel (pixel_format.hip.h)
void launch_pixels_to_bgr(int format, const uint8_t* src, int64_t src_fs, int stride, int w, int h, int n, uint8_t* dst, hipStream_t st);
// n frames of a device frame list (tab_dev: their 3n plane addresses in device memory) gathered into the plan's staged layout at dst,
// frames P.frame_bytes apart: frame_gather_kernel (frame_list.hip.h)
void launch_frame_gather(const FrameListPlan& P, const uint8_t* const* tab_dev, int n, uint8_t* dst, hipStream_t st);
// n BGR8 images of w x h through the matcher's levels table (m->d_levels; fs.levels.set), src == dst with equal strides: in place:
// levels_kernel (levels.hip.h)
void launch_levels(slideo_matcher* m, const uint8_t* src, int64_t src_fs, int src_stride, uint8_t* dst, int64_t dst_fs, int dst_stride, int w, int h,
                   int n, hipStream_t st);
// n BGR8 images of w x h — the field's analysed size — through the matcher's gain field (m->d_shading; fs.shading.set) and, with
// `levels`, through the levels table in the same pass (the fused instance; levels_kernel is then not launched); src == dst with equal
// strides: in place: shading_kernel (shading.hip.h)
void launch_shading(slideo_matcher* m, bool levels, const uint8_t* src, int64_t src_fs, int src_stride, uint8_t* dst, int64_t dst_fs, int dst_stride,
                    int w, int h, int n, hipStream_t st);

// ---- stage_knn.hip --------------------------------------------------------------------------------
// FlannMatcher::new (mo/flann.rs:65-71) for the Hamming index: uploads the M packed rows, collapses equal rows, builds the
// matrix-core operand (and the LSH tables for matcher 1).  Sets m->Mu.
void knn_build_index(slideo_matcher* m, const std::vector<uint8_t>& train, int64_t M);
// A unit's search, decided once from what unit_submit observes (S.knn.shared, S.u_set, the n frames' pixels): rows searched,
// de-duplication, engine, block shape, segments, grid.  Reserves the search's workspace (before the timed interval) and leaves the
// plan in S.knn.  qplan: the query count the launch is planned for, qtot: the capacity (async) or the real count.
void knn_plan_unit(slideo_matcher* m, Slot& S, int n, int64_t frame_pixels, uint32_t qplan, uint32_t qtot);
// the search as S.knn plans it: S.d_desc -> S.d_keys (+ the expansion of the collapsed rows)
void unit_knn(slideo_matcher* m, Slot& S, int n, uint32_t qplan, uint32_t qtot, bool async, bool prof);
bool knn_unit_is_valu(const slideo_matcher* m);
// the {0,1} FP4 expansion of the operand rows perm[0 .. nt_pad) of t (knn_tile.hip.h knn_tile_expand_kernel)
void knn_expand_operand(const uint32_t* t, int nt, int nt_pad, const int32_t* perm, uint4* tx, hipStream_t st);
int knn_operand_rows(int nt);                              // nt padded to whole super-tiles
OperandLayout knn_operand_layout();
std::vector<int32_t> knn_tile_order(int ntiles);           // the fixed pseudo-random order the operand's 32-row tiles are streamed in
void l2_prepare(slideo_matcher::L2Set& L, const uint8_t* t, int nt, hipStream_t st);
void l2_query(slideo_matcher* m, slideo_matcher::L2Set& L, const uint8_t* q_dev, int nq, int k, hipStream_t st, Slot& S, bool timed,
              DevBuf* keys = nullptr, DevBuf* pend = nullptr, float prune_tol = 0.f);
// SIFT matcher mode: the vote rule applied to the L2 lists, as Hamming-format lists in S.d_keys
void l2_lists_to_keys(slideo_matcher* m, Slot& S, const DevBuf& lists, int kq, uint32_t qtot, bool lowe, hipStream_t st);

// ---- stage_verify.hip -----------------------------------------------------------------------------
void verify_stage_init(slideo_matcher* m);
VerifyParams make_vp(const slideo_config& c);
void unit_verify(slideo_matcher* m, Slot& S, const VerifyParams& vp, const DevFrames& f, int n, uint32_t qtot);
// Match evidence map (evidence.hip.h), no-ops without a session.  evidence_admit: in front of a match call's first unit — the
// analysed size against the session's (SLIDEO_ERR_INVALID_ARG), the frames limit, and at the session's first call the zeroed counts.
// evidence_tally: the frame counts of a collected unit from the verdicts it returns.  evidence_drop: the state "none".
void evidence_admit(slideo_matcher* m, int uw, int uh, int n);
void evidence_tally(slideo_matcher* m, const slideo_verdict* v, int n);
inline void evidence_drop(slideo_matcher* m) { m->evidence = slideo_matcher::Evidence{}; }
// Match tone table (tone.hip.h), no-ops without a session.  tone_admit: in front of a match call's first unit, the frames limit.
// tone_tally: the frames of a collected unit.  tone_drop: the state "none".  sessions_drop: what ends an evidence session ends a tone session
void tone_admit(slideo_matcher* m, int n);
inline void tone_tally(slideo_matcher* m, int n) { if (m->tone.on) m->tone.through += n; }
inline void tone_drop(slideo_matcher* m) { m->tone = slideo_matcher::Tone{}; }
// Match placement map (placement.hip.h), no-ops without a session.  placement_admit: evidence_admit's checks and first-call zeroing
// with the limit on the frames through.  placement_tally: the frames of a collected unit.  placement_drop: the state "none"
void placement_admit(slideo_matcher* m, int uw, int uh, int n);
inline void placement_tally(slideo_matcher* m, int n) { if (m->placement.on && m->placement.aw > 0) m->placement.through += n; }
inline void placement_drop(slideo_matcher* m) { m->placement = slideo_matcher::Placement{}; }
// Match shading map (shading.hip.h), no-ops without a session.  shading_map_admit: placement_admit's checks and first-call zeroing,
// and the grid's limit of 4096 cells (SLIDEO_ERR_UNSUPPORTED).  shading_map_tally: the frames of a collected unit
void shading_map_admit(slideo_matcher* m, int uw, int uh, int n);
// every argument and state rule of slideo_matcher_shading_begin (SLIDEO_ERR_INVALID_ARG, _UNSUPPORTED, _STATE), nothing changed
void shading_map_begin_check(slideo_matcher* m, int cell, int min_inliers, int min_hits, int flat);
inline void shading_map_tally(slideo_matcher* m, int n) { if (m->shading_map.on && m->shading_map.aw > 0) m->shading_map.through += n; }
inline void shading_map_drop(slideo_matcher* m) { m->shading_map = slideo_matcher::ShadingMap{}; }
inline void sessions_drop(slideo_matcher* m) { evidence_drop(m); tone_drop(m); placement_drop(m); shading_map_drop(m); }
// (sw, sh: the small size, for callers without a FramePlan — pages, taps, the validity map)
void run_small(slideo_matcher* m, const DevFrames& imgs, int n, hipStream_t st, int* sw = nullptr, int* sh = nullptr);
// the same into `dst` (n small images back to back) in place of m->d_small: small images of consecutive gated units overlap
void run_small_into(slideo_matcher* m, const DevFrames& imgs, int n, DevBuf& dst, hipStream_t st, int* sw = nullptr, int* sh = nullptr);
// ssd[i] = sum of squared differences of the small images a + i * a_stride and b + i * b_stride (`bytes` each), i < n
void launch_ssd(const uint8_t* a, int64_t a_stride, const uint8_t* b, int64_t b_stride, int64_t bytes, unsigned long long* ssd, int n, hipStream_t st);

// ---- stage_page_set.hip ---------------------------------------------------------------------------
// the set's operand from pages[0 .. n) (validated: distinct, in range) on m->stream; the set's id
int page_set_create(slideo_matcher* m, int n, const int32_t* pages);
// a unit's page set (nullptr: the whole deck)
const PageSet* page_set_of(const slideo_matcher* m, int set);
// the frame modes a page set does not cover (SLIDEO_ERR_UNSUPPORTED): checked by use_page_set and by every frame call under a set
void page_set_check_mode(const slideo_matcher* m);

// ---- stage_gate.hip -------------------------------------------------------------------------------
void gate_release(slideo_matcher* m);          // the gate's events (slideo_matcher_destroy)
inline void gate_state_reset(slideo_matcher* m) { m->gate = slideo_matcher::GateState{}; }      // (the gate's own entry points; a setter: settings_commit)
// FrameSrc::staging_bytes' gate_small of a gated call (a small image has at most small_area pixels)
// (under a direct similarity: + the frame's centred operand row, its row of dot products and its record; under the direct scope
// VALID + the masked page norms, 8 bytes per page once per matcher: counted with every frame, a unit has at least one)
// (under SLIDEO_GATE_ANCHOR: + the frame's centred operand row of the pair table, its norm, carried SSD and its row of the table —
// 8 n bytes, n <= GATE_ANCHOR_MAX_UNIT; under a gate settle + the previous frame's small image and the count of the state, and
// the unit's one more carried SSD: counted with every frame, a unit has at least one)
inline size_t gate_small_budget(const slideo_matcher* m) {
    const size_t small = (size_t)m->cfg.small_area * 3 + 64;
    const size_t settle = m->fs.settle_similarity > 0.f ? small + 256 + 32 : 0;
    // (with a gate memory of M: + the frame's row of the n x M table and its ref; the ring and its operand: gate_memory_budget)
    const size_t M = (size_t)m->fs.gate_memory;
    const size_t memory = M > 0 ? 8 * M + 8 : 0;
    const size_t anchor = m->fs.gate_ref == SLIDEO_GATE_ANCHOR ? small + 128 + 32 + (size_t)GATE_ANCHOR_MAX_UNIT * 8 + settle + memory : 0;
    if (!(m->fs.direct_t > 0.f)) return small + anchor;
    const size_t look = 2 * small + 128 + m->pages.size() * 8 + 64 + anchor;
    return m->fs.direct_scope == SLIDEO_DIRECT_VALID ? look + m->pages.size() * 8 : look;
}
// what a gated unit under a gate memory of M takes whatever its frame count ("Gate memory"): the ring's M small images, its centred
// operand of ssd_rows_pad(M) = 64 rows and the unit's record
inline size_t gate_memory_budget(const slideo_matcher* m) {
    const size_t M = m->fs.gate_ref == SLIDEO_GATE_ANCHOR ? (size_t)m->fs.gate_memory : 0;
    return M > 0 ? (M + 64) * ((size_t)m->cfg.small_area * 3 + 64 + 128) + 2048 : 0;
}
// a validated source's frames against a gate state (m->gate, the N-device group's): one size and one format family since the last
// reset (SLIDEO_ERR_STATE)
void gate_check(const slideo_matcher::GateState& g, const FrameSrc& src);
// slideo_matcher_gate_reset_from_frame_*: the gate state of an idle matcher := the small image of the ONE frame of src (frame_stride
// as of a single frame), staged as a gated unit stages it; user_stream: the stream a device frame was produced on
void gate_prime(slideo_matcher* m, FrameSrc src, hipStream_t user_stream);
// The gate state's device buffers (include/slideo_amd.h "Gate state record"): gate_state_read copies the anchor (sb bytes) and, under
// a settle, the previous image and the deferral count to host memory behind `behind` (may be null) on the matcher's copy stream, and
// waits for them; gate_state_write reserves the buffers and queues the opposite copies on st (the host memory stays valid and
// unchanged until st has run them).
void gate_state_read(slideo_matcher* m, hipEvent_t behind, size_t sb, uint8_t* anchor, uint8_t* prev, uint32_t* d);
void gate_state_write(slideo_matcher* m, size_t sb, const uint8_t* anchor, const uint8_t* prev, const uint32_t* d, hipStream_t st);
// the pending hand-over of a chained group call, where a gated unit waits for the state (no-op on a single matcher)
inline void gate_chain_receive(slideo_matcher* m, hipStream_t st) {
    if (!m->gate_receive) return;
    const std::function<void(hipStream_t)> f = std::move(m->gate_receive);
    m->gate_receive = nullptr;
    f(st);
}
// One gated unit on slot S: frames [first, first + n) of src through the gate, the changed ones through unit_submit (S.n = their
// count, 0: no pipeline ran); its collect: flags and similarities of all n frames, verdicts of the changed ones
void gate_unit_submit(slideo_matcher* m, Slot& S, const FrameSrc& src, int first, int n, hipStream_t cs);
void gate_unit_collect(slideo_matcher* m, Slot& S, uint8_t* changed_out, float* similarity_out, slideo_verdict* verdicts_out);

// Frame mask scope (include/slideo_amd.h "Frame mask scope").  gate_map_build: the validity map of the w x h mask at dmask (DEVICE
// memory, rows `pitch` apart) into `out` and its weights `out_w`, on m->stream (SLIDEO_ERR_INVALID_ARG when no small pixel is valid).
// gate_map_for: the weights a call that makes changed flags from frames of analysed size w x h sums its
// SSDs under, *npx the pixels its similarities are normalised over — nullptr and sw * sh unless a mask is set under the GATE scope;
// SLIDEO_ERR_INVALID_ARG at another size than the mask's.
void gate_map_build(slideo_matcher* m, const uint8_t* dmask, int pitch, int w, int h, GateMap& out, DevBuf& out_w);
const uint8_t* gate_map_for(const slideo_matcher* m, int w, int h, int sw, int sh, int* npx);
// launch_ssd, under `weights` (gate_map_for) when not null
void launch_gate_ssd(const uint8_t* weights, const uint8_t* a, int64_t a_stride, const uint8_t* b, int64_t b_stride, int64_t bytes,
                     unsigned long long* ssd, int n, hipStream_t st);
// the smallest SSD that counts as changed when the similarity is normalised over n pixels (slideo_changed_ssd_threshold_n)
int64_t gate_ssd_threshold(float changed_similarity_, int64_t n);

// ---- stage_direct.hip -----------------------------------------------------------------------------
// the largest SSD whose host similarity over n pixels is >= t (slideo_direct_ssd_threshold; -1: none)
int64_t direct_ssd_threshold(float t, int64_t n);
// What a gated unit of n frames with sw x sh small images looks up in: everything that can fail for want of memory — the page
// operand at its first use, the selected set's eligible list, the slot's workspaces — happens here, in front of any change to the
// gate state.  cls == null: no page of the set shares the small size, the unit does not look up.
// weights: the gate's validity map (gate_map_for) under SLIDEO_DIRECT_VALID, null otherwise: the look-up then runs over the valid
// bytes — the frames' operand masked, bnorm the class's masked page norms (built here when the map's generation has moved on).
struct DirectPlan {
    const DirectClass* cls = nullptr; const int32_t* elig = nullptr; int ne = 0;
    const uint8_t* weights = nullptr; const long long* bnorm = nullptr;
};
DirectPlan direct_unit_prepare(slideo_matcher* m, Slot& S, int n, int sw, int sh, const uint8_t* weights);
// The look-up on S.st, behind the unit's small images (S.d_gsmall) and in front of gate_kernel: the frames' operand,
// page_ssd_kernel over all n frames, direct_best_kernel over the eligible pages.  Launches only.
void direct_unit_lookup(Slot& S, const DirectPlan& plan, int n);
// behind gate_kernel: direct_gate_kernel on the unit's kept list idx / count, the record's tail at h_rec, the list's pinned twin h_idx
void direct_unit_gate(slideo_matcher* m, Slot& S, int n, int npx, int32_t* idx, uint32_t* count, int32_t* h_idx, uint8_t* h_rec);
size_t direct_unit_rec_bytes(int n);
// one frame's entry of the record's tail
struct DirectFrameRec { unsigned long long ssd; int32_t page; bool direct; };
uint32_t direct_rec_kept(const uint8_t* h_rec, int n);
DirectFrameRec direct_rec_frame(const uint8_t* h_rec, int n, int i);

// ---- stage_ssd_table.hip --------------------------------------------------------------------------
int64_t ssd_kp(int64_t L);                  // bytes of an operand row for small images of L bytes
int ssd_rows_pad(int rows);                 // operand rows for `rows` images
// The centred operand `out` ([rows_pad][kp], ssd_table.hip.h's layout) and the norms |x'|^2 of the n images of L bytes at
// src + (ofs ? ofs[row] : row * stride), on st.  weights (the gate's validity map): the operand zero at the masked bytes, the norms
// over the valid ones; out null (weights only): the norms alone
void ssd_operand_build(const uint8_t* src, int64_t stride, const long long* ofs, int n, int rows_pad, int64_t L, int64_t kp, uint4* out,
                       long long* norm, hipStream_t st, const uint8_t* weights = nullptr);
// dot[i * np + j] = <a'_i, b'_j> of the operands a (n rows) and b (np rows), on st (page_ssd_kernel); b null: the symmetric table of
// a, dot[i * n + j] for i < j alone (frame_gram_kernel).  Launches only.
void ssd_table_dots(const uint4* a, int n, const uint4* b, int np, int64_t kp, unsigned long long* dot, hipStream_t st);
// the weights a tap sums under: null unless use_valid, then the matcher's validity map — SLIDEO_ERR_STATE when none is in force,
// SLIDEO_ERR_INVALID_ARG when it is not sw x sh (`tap`: the name the message begins with)
const uint8_t* tap_valid_weights(const slideo_matcher* m, const char* tap, bool use_valid, int sw, int sh);

// ---- stage_gate_anchor.hip ------------------------------------------------------------------------
// Where gate_anchor_unit writes a unit's decisions: gate_kernel's outputs — device flags, kept list and count, and the pinned
// record's header {count, n}, SSDs, kept list and flags (gate.hip.h GateHostRec and gate_rec_*)
struct GateAnchorOut {
    uint8_t* flags; int32_t* idx; uint32_t* count;
    uint32_t* h_head; unsigned long long* h_ssd; int32_t* h_idx; uint8_t* h_flag;
};
// a unit of n frames with sw x sh small images under SLIDEO_GATE_ANCHOR: S's workspaces and, with a settle in force, the matcher's
// previous-frame image and deferral count (everything that can fail for want of memory, in front of any write of the gate state)
// memory: the gate memory's capacity in force (0: none) — + the matcher's ring and the slot's workspaces of "Gate memory"
void gate_anchor_reserve(slideo_matcher* m, Slot& S, int n, int sw, int sh, bool settle, int memory = 0);
// The unit's gate under SLIDEO_GATE_ANCHOR on S.st, behind the unit's small images `small` (sb bytes each): operand, pair table, then
// behind `wait` (the previous gated unit's event) ONE launch for the n SSDs against the carried anchor m->d_gate_small and, under a
// settle, frame 0's against the carried previous frame (none when force0), the walk, and the new state — the anchor and, under a
// settle (m->fs.settle_similarity > 0; thr_s: its SSD threshold, max_defer: its cap), the previous frame and the deferral count.
// Without a settle thr_s = 0 and max_defer = 0: a frame away from its anchor is matched at once.  Launches only.
void gate_anchor_unit(slideo_matcher* m, Slot& S, const uint8_t* weights, const uint8_t* small, int64_t sb, int n, long long thr, long long thr_s,
                      int32_t max_defer, bool force0, hipEvent_t wait, const GateAnchorOut& out);
// its first step alone: operand, norms (S.d_ga_rec's first n i64) and the table S.d_ga_dot[i * n + j], i < j, of the n small images at
// `small` (L bytes each), on st; S reserved by gate_anchor_reserve
void gram_launch(Slot& S, const uint8_t* weights, const uint8_t* small, int64_t L, int n, hipStream_t st);
// the previous-frame image := the anchor's (m->d_gate_small, sb bytes) and the deferral count := 0, on st: what every reset of the
// gate state to an image does under a settle
void gate_settle_state_from_anchor(slideo_matcher* m, size_t sb, hipStream_t st);
// with a gate memory in force: the ring := [(the anchor's image m->d_gate_small, SLIDEO_GATE_REF_RESET)], anchor slot 0, d = 0, on st
// (reserves the ring: every allocation in front of the first write); what every reset of the gate state to an image does
void gate_memory_state_from_anchor(slideo_matcher* m, size_t sb, hipStream_t st);
// the anchor's small image (sb bytes) of the ring -> out (host), behind everything queued; idle matcher, state not "none"
void gate_memory_read_anchor(slideo_matcher* m, size_t sb, uint8_t* out);

// ---- stage_sift.hip -------------------------------------------------------------------------------
void sift_check_cfg(const slideo_sift_config* sc, int w, int h);
void unit_submit_sift(slideo_matcher* m, Slot& S, const DevFrames& f, int n);
void add_pages_sift(slideo_matcher* m, Slot& S, const DevFrames& pages, int cnt);

}  // namespace slideo

#define API_TRY try {
#define API_CATCH(m)                                                          \
    }                                                                         \
    catch (const slideo::Error& e) { slideo::set_err(m, e.what()); return e.code; }   \
    catch (const std::exception& e) { slideo::set_err(m, e.what()); return SLIDEO_ERR_HIP; } \
    catch (...) { slideo::set_err(m, "unknown error"); return SLIDEO_ERR_HIP; }       \
    return SLIDEO_OK;

// A matcher's set call as its entry point's return code: propose(fs) — frame_settings.h propose_* — into settings_commit
template <class Propose>
int32_t matcher_set(slideo_matcher* m, slideo::Setting what, Propose propose, const uint8_t* mask = nullptr, int stride = 0) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    slideo::settings_commit(m, what, propose(m->fs), mask, stride);
    API_CATCH(m)
}
