// stage_verify.hip — drivers of the verification stage, vote .. verdict, and of to_small_image (kernels: verify.hip.h, homography.hip.h);
// the match evidence map of include/slideo_amd.h "Match evidence map": its session, its launch behind the verdicts and its entry
// points (kernel: evidence.hip.h); the match tone table of "Match tone table" likewise (kernel: tone.hip.h), and the match placement map of
// "Match placement map" (kernel: placement.hip.h).
#include "runtime.hpp"
#include "verify.hip.h"
#include "homography.hip.h"
#include "evidence.hip.h"
#include "tone.hip.h"
#include "placement.hip.h"
#include "placement_lens.h"
#define SHADING_MAP              // (shading_kernel is stage_orb.hip's)
#include "shading.hip.h"

#include <cstring>

using namespace slideo;

namespace slideo {

VerifyParams make_vp(const slideo_config& c) {
    VerifyParams v{};
    v.k = c.knn_k; v.klist = KLIST; v.max_cand = c.max_candidate_pages; v.max_rated = c.max_rated;
    v.tol = c.vote_tolerance; v.min_similarity = c.min_similarity; v.ratio = c.ratio_test;
    v.thr = c.ransac_threshold; v.conf = c.ransac_confidence; v.min_rating = c.min_rating;
    v.min_rating_ratio = c.min_rating_ratio; v.max_iters = c.ransac_max_iters; v.refine_iters = c.refine_iters;
    v.model = c.verify_model; v.verdict_rule = c.verdict_rule;
    v.sched_window = env_long("SLIDEO_RANSAC_WINDOW", 1) != 0;      // (read per unit: the tests switch it)
    return v;
}

// ---- to_small_image of n equally sized device images into m->d_small --------------------
void run_small(slideo_matcher* m, const DevFrames& imgs, int n, hipStream_t st, int* sw, int* sh) {
    run_small_into(m, imgs, n, m->d_small, st, sw, sh);
}

void run_small_into(slideo_matcher* m, const DevFrames& imgs, int n, DevBuf& dst, hipStream_t st, int* sw_out, int* sh_out) {
    int ac = area_class_for(m, imgs.w, imgs.h);
    upload_area(m);
    const AreaGeom& ag = m->area_geoms[ac];
    const int sw = ag.dw, sh = ag.dh;
    if (sw_out) { *sw_out = sw; *sh_out = sh; }
    dst.reserve((size_t)n * sw * sh * 3);
    int tiles = cdiv(sw, SM_TW) * cdiv(sh, SM_TH);
    small_image_kernel<<<dim3(tiles, n), 256, 0, st>>>(ag, m->d_area_taps.as<AreaTap>(), m->d_area_idx.as<int32_t>(), imgs.p,
                                                       imgs.frame_stride, imgs.stride, dst.as<uint8_t>(), (int64_t)sw * sh * 3);
    check_launch("small_image_kernel");
}

void launch_ssd(const uint8_t* a, int64_t a_stride, const uint8_t* b, int64_t b_stride, int64_t bytes, unsigned long long* ssd, int n, hipStream_t st) {
    ssd_kernel<<<n, 256, 0, st>>>(a, a_stride, b, b_stride, bytes, ssd);
    check_launch("ssd_kernel");
}

// ---- match evidence map -----------------------------------------------------------------------------------------------------------
void evidence_admit(slideo_matcher* m, int uw, int uh, int n) {
    slideo_matcher::Evidence& E = m->evidence;
    if (!E.on || n <= 0) return;
    if (E.aw > 0 && (E.aw != uw || E.ah != uh))
        fail(SLIDEO_ERR_INVALID_ARG, "these frames are analysed at %dx%d, the evidence session counts at %dx%d: slideo_matcher_evidence_end first", uw, uh,
             E.aw, E.ah);
    int64_t pending = 0;
    for (const Slot& S : m->slots) if (S.busy) pending += S.n;
    if (E.counted + pending + n > E.max_frames)
        fail(SLIDEO_ERR_INVALID_ARG, "%lld frames would pass the evidence session's %lld: read the counts out and begin again", (long long)(E.counted + pending + n),
             (long long)E.max_frames);
    if (E.aw > 0) return;
    // the session's first counted call fixes the grid; the zeroed counts stand before any unit of the call is submitted
    const int gw = cdiv(uw, E.cell), gh = cdiv(uh, E.cell);
    const size_t bytes = (size_t)gw * gh * 8;
    m->d_evidence.reserve(bytes + 16);
    HIP_CHECK(hipMemsetAsync(m->d_evidence.p, 0, bytes, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    E.aw = uw; E.ah = uh; E.gw = gw; E.gh = gh;
}

void evidence_tally(slideo_matcher* m, const slideo_verdict* v, int n) {
    slideo_matcher::Evidence& E = m->evidence;
    if (!E.on || E.aw == 0) return;
    E.through += n;
    for (int i = 0; i < n; ++i) E.counted += v[i].page_idx >= 0 && v[i].inliers >= E.min_inliers;
}

// evidence_kernel over the unit's frames, behind verdict_kernel on the unit's stream
static void evidence_launch(slideo_matcher* m, Slot& S, const VerifyParams& vp, const DevFrames& f, int n) {
    const slideo_matcher::Evidence& E = m->evidence;
    if (E.aw != f.w || E.ah != f.h) fail(SLIDEO_ERR_HIP, "internal: a unit of %dx%d images under an evidence session of %dx%d", f.w, f.h, E.aw, E.ah);
    EvidenceArgs a{};
    a.verdicts = S.d_verdicts.as<slideo_verdict>(); a.fcs = S.d_fcs.as<FrameCands>(); a.qofs = S.d_qofs.as<uint32_t>();
    a.kp = S.d_kp.as<slideo_keypoint>();
    a.page_xy = reinterpret_cast<const EvXY*>(m->d_page_xy.as<float2>());
    a.votes = reinterpret_cast<const EvVote*>(S.d_votes.as<uint2>());
    a.flags = S.d_flags.as<uint32_t>();
    a.rerun_mask = S.u_async ? 12u : 4u;      // unit_collect's re-run rules: the RNG stream; the keypoint capacity of the capacity-sized path
    a.k = vp.k; a.model = vp.model; a.min_inliers = E.min_inliers; a.thr2 = vp.thr * vp.thr;
    a.aw = E.aw; a.ah = E.ah; a.cell = E.cell; a.gw = E.gw; a.gh = E.gh;
    a.seen = m->d_evidence.as<uint32_t>(); a.hit = a.seen + (size_t)E.gw * E.gh;
    evidence_kernel<<<n, EV_THREADS, 0, S.st>>>(a);
    check_launch("evidence_kernel");
}

// ---- match tone table ---------------------------------------------------------------------------------------------------------------
void tone_admit(slideo_matcher* m, int n) {
    const slideo_matcher::Tone& T = m->tone;
    if (!T.on || n <= 0) return;
    int64_t pending = 0;
    for (const Slot& S : m->slots) if (S.busy) pending += S.n;
    if (T.through + pending + n > T.max_frames)
        fail(SLIDEO_ERR_INVALID_ARG, "%lld frames would pass the tone session's %lld: read the counts out and begin again", (long long)(T.through + pending + n),
             (long long)T.max_frames);
}

// tone_kernel over the unit's frames, behind verdict_kernel (and evidence_kernel) on the unit's stream
static void tone_launch(slideo_matcher* m, Slot& S, const VerifyParams& vp, const DevFrames& f, int n) {
    const slideo_matcher::Tone& T = m->tone;
    ToneArgs a{};
    a.ev.fcs = S.d_fcs.as<FrameCands>(); a.ev.qofs = S.d_qofs.as<uint32_t>(); a.ev.kp = S.d_kp.as<slideo_keypoint>();
    a.ev.page_xy = reinterpret_cast<const EvXY*>(m->d_page_xy.as<float2>());
    a.ev.votes = reinterpret_cast<const EvVote*>(S.d_votes.as<uint2>());
    a.ev.flags = S.d_flags.as<uint32_t>();
    a.ev.rerun_mask = S.u_async ? 12u : 4u;      // (evidence_launch's: unit_collect's re-run rules)
    a.ev.k = vp.k; a.ev.model = vp.model; a.ev.thr2 = vp.thr * vp.thr;
    a.pageinfo = m->d_pageinfo.as<PageInfo>(); a.page_small = m->d_page_small.as<uint8_t>();
    a.frames = f.p; a.frame_stride = f.frame_stride; a.stride = f.stride; a.aw = f.w; a.ah = f.h;
    a.min_inliers = T.min_inliers; a.min_hits = T.min_hits; a.flat = T.flat;
    a.acc = m->d_tone.as<unsigned long long>();
    tone_kernel<<<n, TONE_THREADS, 0, S.st>>>(a);
    check_launch("tone_kernel");
}

// ---- match placement map ----------------------------------------------------------------------------------------------------------
void placement_admit(slideo_matcher* m, int uw, int uh, int n) {
    slideo_matcher::Placement& P = m->placement;
    if (!P.on || n <= 0) return;
    if (P.aw > 0 && (P.aw != uw || P.ah != uh))
        fail(SLIDEO_ERR_INVALID_ARG, "these frames are analysed at %dx%d, the placement session counts at %dx%d: slideo_matcher_placement_end first", uw, uh,
             P.aw, P.ah);
    int64_t pending = 0;
    for (const Slot& S : m->slots) if (S.busy) pending += S.n;
    if (P.through + pending + n > P.max_frames)
        fail(SLIDEO_ERR_INVALID_ARG, "%lld frames would pass the placement session's %lld: read the sums out and begin again", (long long)(P.through + pending + n),
             (long long)P.max_frames);
    if (P.aw > 0) return;
    // the session's first counted call fixes the grid; the zeroed sums stand before any unit of the call is submitted
    const int gw = cdiv(uw, P.cell), gh = cdiv(uh, P.cell);
    const size_t bytes = ((size_t)gw * gh * 5 + 1) * 8;
    m->d_placement.reserve(bytes + 16);
    HIP_CHECK(hipMemsetAsync(m->d_placement.p, 0, bytes, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    P.aw = uw; P.ah = uh; P.gw = gw; P.gh = gh;
}

// placement_kernel over the unit's frames, behind verdict_kernel (and evidence_kernel, tone_kernel) on the unit's stream
static void placement_launch(slideo_matcher* m, Slot& S, const VerifyParams& vp, const DevFrames& f, int n) {
    const slideo_matcher::Placement& P = m->placement;
    if (P.aw != f.w || P.ah != f.h) fail(SLIDEO_ERR_HIP, "internal: a unit of %dx%d images under a placement session of %dx%d", f.w, f.h, P.aw, P.ah);
    PlacementArgs a{};
    a.ev.fcs = S.d_fcs.as<FrameCands>(); a.ev.qofs = S.d_qofs.as<uint32_t>(); a.ev.kp = S.d_kp.as<slideo_keypoint>();
    a.ev.page_xy = reinterpret_cast<const EvXY*>(m->d_page_xy.as<float2>());
    a.ev.votes = reinterpret_cast<const EvVote*>(S.d_votes.as<uint2>());
    a.ev.flags = S.d_flags.as<uint32_t>();
    a.ev.rerun_mask = S.u_async ? 12u : 4u;      // (evidence_launch's: unit_collect's re-run rules)
    a.ev.k = vp.k; a.ev.model = vp.model;
    a.pageinfo = m->d_pageinfo.as<PageInfo>();
    a.reach2 = P.reach * P.reach;
    a.aw = P.aw; a.ah = P.ah; a.cell = P.cell; a.gw = P.gw; a.gh = P.gh; a.min_inliers = P.min_inliers;
    a.acc = m->d_placement.as<unsigned long long>();
    placement_kernel<<<n, PL_THREADS, 0, S.st>>>(a);
    check_launch("placement_kernel");
}

// ---- match shading map --------------------------------------------------------------------------------------------------------------
void shading_map_admit(slideo_matcher* m, int uw, int uh, int n) {
    slideo_matcher::ShadingMap& H = m->shading_map;
    if (!H.on || n <= 0) return;
    if (H.aw > 0 && (H.aw != uw || H.ah != uh))
        fail(SLIDEO_ERR_INVALID_ARG, "these frames are analysed at %dx%d, the shading session counts at %dx%d: slideo_matcher_shading_end first", uw, uh,
             H.aw, H.ah);
    int64_t pending = 0;
    for (const Slot& S : m->slots) if (S.busy) pending += S.n;
    if (H.through + pending + n > H.max_frames)
        fail(SLIDEO_ERR_INVALID_ARG, "%lld frames would pass the shading session's %lld: read the sums out and begin again", (long long)(H.through + pending + n),
             (long long)H.max_frames);
    if (H.aw > 0) return;
    // the session's first counted call fixes the grid; the zeroed sums stand before any unit of the call is submitted
    const int gw = cdiv(uw, H.cell), gh = cdiv(uh, H.cell);
    if ((int64_t)gw * gh > SHM_MAX_CELLS)
        fail(SLIDEO_ERR_UNSUPPORTED, "a shading session of %dx%d cells (%dx%d at cell %d): at most %d cells, which cell %d gives", gw, gh, uw, uh, H.cell,
             SHM_MAX_CELLS, H.cell * 2);
    const size_t bytes = ((size_t)gw * gh * 3 + 1) * 8;
    m->d_shading_map.reserve(bytes + 16);
    HIP_CHECK(hipMemsetAsync(m->d_shading_map.p, 0, bytes, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    H.aw = uw; H.ah = uh; H.gw = gw; H.gh = gh;
}

// what slideo_matcher_shading_begin refuses (the group's begin runs it over every member before it touches one)
void shading_map_begin_check(slideo_matcher* m, int cell, int min_inliers, int min_hits, int flat) {
    if (!evidence_cell_ok(cell)) fail(SLIDEO_ERR_INVALID_ARG, "shading_begin: cell %d is none of 16, 32, 64", cell);
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "shading_begin: min_inliers %d below 0", min_inliers);
    if (min_hits < 1) fail(SLIDEO_ERR_INVALID_ARG, "shading_begin: min_hits %d below 1", min_hits);
    if (flat < 0 || flat > 255) fail(SLIDEO_ERR_INVALID_ARG, "shading_begin: flat %d outside 0..255", flat);
    if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "shading_begin: the shading map is not defined in SIFT mode");
    require_idle(m);
    if (m->shading_map.on) fail(SLIDEO_ERR_STATE, "shading_begin: a session is open (slideo_matcher_shading_end first)");
    if (m->fs.shading.set)
        fail(SLIDEO_ERR_STATE, "shading_begin: a frame shading is set, and a field learnt on shaded frames is not the source's "
                               "(slideo_matcher_set_frame_shading(m, 0, 0, 0, NULL) first)");
    if (m->fs.levels.set)
        fail(SLIDEO_ERR_STATE, "shading_begin: a frame levels table is set, and a gain learnt behind the table cannot be installed in front of it: "
                               "learn the field first and the table second (slideo_matcher_set_frame_levels(m, NULL) first)");
}

// shading_map_kernel over the unit's frames, behind verdict_kernel and the other sessions' kernels on the unit's stream
static void shading_map_launch(slideo_matcher* m, Slot& S, const VerifyParams& vp, const DevFrames& f, int n) {
    const slideo_matcher::ShadingMap& H = m->shading_map;
    if (H.aw != f.w || H.ah != f.h) fail(SLIDEO_ERR_HIP, "internal: a unit of %dx%d images under a shading session of %dx%d", f.w, f.h, H.aw, H.ah);
    ShadingMapArgs a{};
    a.t.ev.fcs = S.d_fcs.as<FrameCands>(); a.t.ev.qofs = S.d_qofs.as<uint32_t>(); a.t.ev.kp = S.d_kp.as<slideo_keypoint>();
    a.t.ev.page_xy = reinterpret_cast<const EvXY*>(m->d_page_xy.as<float2>());
    a.t.ev.votes = reinterpret_cast<const EvVote*>(S.d_votes.as<uint2>());
    a.t.ev.flags = S.d_flags.as<uint32_t>();
    a.t.ev.rerun_mask = S.u_async ? 12u : 4u;    // (evidence_launch's: unit_collect's re-run rules)
    a.t.ev.k = vp.k; a.t.ev.model = vp.model; a.t.ev.thr2 = vp.thr * vp.thr;
    a.t.pageinfo = m->d_pageinfo.as<PageInfo>(); a.t.page_small = m->d_page_small.as<uint8_t>();
    a.t.frames = f.p; a.t.frame_stride = f.frame_stride; a.t.stride = f.stride; a.t.aw = f.w; a.t.ah = f.h;
    a.t.min_inliers = H.min_inliers; a.t.min_hits = H.min_hits; a.t.flat = H.flat;
    a.shift = H.cell == 16 ? 4 : H.cell == 32 ? 5 : 6; a.gw = H.gw; a.cells = H.gw * H.gh;
    a.acc = m->d_shading_map.as<unsigned long long>();
    shading_map_kernel<<<n, TONE_THREADS, ((size_t)a.cells * 3 + 5) * sizeof(uint32_t), S.st>>>(a);
    check_launch("shading_map_kernel");
}

// Everything after the neighbour lists (S.d_keys, Hamming key format) of a unit: the per-page vote, RANSAC (similarity or
// homography), rating, re-projection, verdicts, and the unit's one D2H copy.  `f`: the unit's frames (re-projection).
void unit_verify(slideo_matcher* m, Slot& S, const VerifyParams& vp, const DevFrames& f, int n, uint32_t qtot) {
    const slideo_config& c = m->cfg;
    hipStream_t st = S.st;
    const bool prof = m->profiling;
    const int P = (int)m->pages.size();
    uint32_t* flags = S.d_flags.as<uint32_t>();
    if (qtot > 0) {
        const size_t lds = (size_t)P * 4 + (((size_t)P + 15) & ~(size_t)15) + (size_t)c.max_candidate_pages * 256 * 4;
        vote_kernel<<<n, 256, lds, st>>>(vp, S.d_keys.as<uint32_t>(), S.d_qofs.as<uint32_t>(), m->d_train_page.as<int32_t>(), P,
                                         S.d_fcs.as<FrameCands>(), S.d_votes.as<uint2>());
        check_launch("vote_kernel");
        if (c.verify_model == 1) {
            // hdlt >= 1: a candidate still sampling after `round_cap` rounds goes to ransac_h_tail_kernel (8 waves on its sample
            // schedule).  hdlt 0 is bound by its eigen-solver, not by the schedule: no cap.  flags[1] counts the tail list, flags[2] hands it out (flags[3]: refine_h's eigenproblem list).
            const long tail_env = env_long("SLIDEO_RH_TAIL_ROUNDS", 256);                     // (read per unit: the tests switch it)
            const uint32_t tail_rounds = (uint32_t)(tail_env < 1 ? 0xFFFFFFFFu : tail_env);   // 0 / negative: never hand over
            const uint32_t round_cap = c.ocv.hdlt ? tail_rounds : 0xFFFFFFFFu;
            S.d_tail.reserve((size_t)c.max_candidate_pages * n * 4 + 16);
            auto launch_h = [&](auto small_tag, auto large_tag, int hdlt) {
                small_tag<<<dim3(c.max_candidate_pages, n), 64, ransac_h_lds_bytes(RANSAC_SMALL_PTS, hdlt), st>>>(
                    vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
                    m->d_rng.as<uint32_t>(), S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), flags, round_cap,
                    S.d_tail.as<uint32_t>(), flags + 1);
                check_launch("ransac_h_kernel (small)");
                large_tag<<<dim3(c.max_candidate_pages, n), 64, ransac_h_lds_bytes(RANSAC_LDS_PTS, hdlt), st>>>(
                    vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
                    m->d_rng.as<uint32_t>(), S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), flags, round_cap,
                    S.d_tail.as<uint32_t>(), flags + 1);
                check_launch("ransac_h_kernel (large)");
            };
            auto launch_tail = [&](auto tail_tag) {
                const int blocks = std::min(RANSAC_H_TAIL_BLOCKS, c.max_candidate_pages * n);
                tail_tag<<<blocks, 64 * RANSAC_H_TAIL_WAVES, ransac_h_tail_lds_bytes(RANSAC_H_TAIL_WAVES), st>>>(
                    vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
                    m->d_rng.as<uint32_t>(), S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), flags,
                    S.d_tail.as<uint32_t>(), flags + 1, flags + 2);
                check_launch("ransac_h_tail_kernel");
            };
            if (c.ocv.hdlt == 2) {
                launch_h(&ransac_h_kernel<RANSAC_SMALL_PTS, 0, 2>, &ransac_h_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1, 2>, 2);
                if (round_cap != 0xFFFFFFFFu) launch_tail(&ransac_h_tail_kernel<2, RANSAC_H_TAIL_WAVES>);
            } else if (c.ocv.hdlt == 1) {
                launch_h(&ransac_h_kernel<RANSAC_SMALL_PTS, 0, 1>, &ransac_h_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1, 1>, 1);
                if (round_cap != 0xFFFFFFFFu) launch_tail(&ransac_h_tail_kernel<1, RANSAC_H_TAIL_WAVES>);
            } else launch_h(&ransac_h_kernel<RANSAC_SMALL_PTS, 0, 0>, &ransac_h_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1, 0>, 0);
            if (c.refine_iters > 0) {
                // runKernel over the inliers: normalise + L^T L (wave per candidate), the eigenproblems 32 per wave, then the LM
                const size_t ncand = (size_t)c.max_candidate_pages * n;
                S.d_refine.reserve(ncand * sizeof(RefineRec) + ncand * 4 + 16);
                RefineRec* recs = S.d_refine.as<RefineRec>();
                uint32_t* eig_list = reinterpret_cast<uint32_t*>(S.d_refine.as<uint8_t>() + ncand * sizeof(RefineRec));
                refine_h_kernel<0><<<dim3(c.max_candidate_pages, n), 64, 0, st>>>(
                    vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
                    S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), recs, eig_list, flags + 3);
                check_launch("refine_h_kernel<0>");
                // the small candidates' LM in the eigen kernel's lanes: less wave time (3.7 -> 2.1 s per headline unit) but a longer
                // critical path (one lane's ten iterations, ~2 ms) — it pays when the candidates outnumber the resident waves
                const int lane_lm = (int)env_long("SLIDEO_REFINE_LANE_LM", ncand >= 4096 ? 1 : 0);      // (read per unit: the tests switch it)
                refine_h_eigen_kernel<<<cdiv((int)ncand, HJ), 64, refine_h_eigen_lds_bytes(), st>>>(
                    vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
                    S.d_fcs.as<FrameCands>(), S.d_gmask.as<uint8_t>(), c.max_candidate_pages, recs, eig_list, flags + 3, lane_lm);
                check_launch("refine_h_eigen_kernel");
                refine_h_kernel<1><<<dim3(c.max_candidate_pages, n), 64, 0, st>>>(
                    vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
                    S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), recs, eig_list, flags + 3);
                check_launch("refine_h_kernel<1>");
            }
        } else {
        ransac_kernel<RANSAC_SMALL_PTS, 0><<<dim3(c.max_candidate_pages, n), 64, 0, st>>>(
            vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
            m->d_rng.as<uint32_t>(), S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), flags);
        check_launch("ransac_kernel (small)");
        ransac_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1><<<dim3(c.max_candidate_pages, n), 64, 0, st>>>(
            vp, S.d_qofs.as<uint32_t>(), S.d_kp.as<slideo_keypoint>(), m->d_page_xy.as<float2>(), S.d_votes.as<uint2>(),
            m->d_rng.as<uint32_t>(), S.d_fcs.as<FrameCands>(), S.d_gpts.as<float4>(), S.d_gmask.as<uint8_t>(), flags);
        check_launch("ransac_kernel (large)");
        }
        uint32_t* pair_count = S.d_pairs.as<uint32_t>();
        PairDesc* pair_list = reinterpret_cast<PairDesc*>(S.d_pairs.as<uint8_t>() + 64);
        HIP_CHECK(hipMemsetAsync(pair_count, 0, 16, st));
        rate_kernel<<<n, 64, 0, st>>>(vp, n, S.d_fcs.as<FrameCands>(), m->d_pageinfo.as<PageInfo>(), pair_list, pair_count);
        check_launch("rate_kernel");
        // the pairs of size classes inside reproject_vt_kernel's limits go through the warped-image tile, the others through the
        // frame window of reproject_kernel (each kernel skips the other's pairs; the second launch only if such a class exists)
        int max_tile_rows = 0;
        bool any_vt = false, any_win = false;
        for (const AreaGeom& ag : m->area_geoms) {
            max_tile_rows = std::max(max_tile_rows, cdiv(ag.dh, SM_TH));
            const bool vt = ag.vt_ok && cdiv(ag.dw, SM_TW) <= RP_MAX_TILES;
            any_vt |= vt; any_win |= !vt;
        }
        const dim3 rgrid(max_tile_rows, std::min(n, 65535));
#define SLIDEO_RP_TAIL m->d_page_small.as<uint8_t>(), f.p, f.frame_stride, f.stride, f.w, f.h, S.d_fcs.as<FrameCands>(), pair_list, pair_count
#define SLIDEO_RP_ARGS m->d_area_geoms.as<AreaGeom>(), m->d_area_taps.as<AreaTap>(), m->d_area_idx.as<int32_t>(), SLIDEO_RP_TAIL
#define SLIDEO_VT_ARGS m->d_area_geoms.as<AreaGeom>(), m->d_area_taps.as<AreaTap>(), m->d_area_idx.as<int32_t>(), m->d_area_recs.as<AreaRec>(), SLIDEO_RP_TAIL
        if (any_vt) {
            if (c.verify_model == 1) reproject_vt_kernel<true><<<rgrid, 256, 0, st>>>(SLIDEO_VT_ARGS);
            else reproject_vt_kernel<false><<<rgrid, 256, 0, st>>>(SLIDEO_VT_ARGS);
            check_launch("reproject_vt_kernel");
        }
        if (any_win) {
            if (c.verify_model == 1) reproject_kernel<true><<<rgrid, 256, 0, st>>>(SLIDEO_RP_ARGS);
            else reproject_kernel<false><<<rgrid, 256, 0, st>>>(SLIDEO_RP_ARGS);
            check_launch("reproject_kernel");
        }
#undef SLIDEO_RP_ARGS
#undef SLIDEO_VT_ARGS
#undef SLIDEO_RP_TAIL
    }
    verdict_kernel<<<cdiv(n, 64), 64, 0, st>>>(vp, n, S.d_qofs.as<uint32_t>(), m->d_pageinfo.as<PageInfo>(), S.d_fcs.as<FrameCands>(),
                                               S.d_verdicts.as<slideo_verdict>());
    check_launch("verdict_kernel");
    if (m->evidence.on && qtot > 0) evidence_launch(m, S, vp, f, n);
    if (m->tone.on && qtot > 0) tone_launch(m, S, vp, f, n);
    if (m->placement.on && qtot > 0) placement_launch(m, S, vp, f, n);
    if (m->shading_map.on && qtot > 0) shading_map_launch(m, S, vp, f, n);
    if (prof) HIP_CHECK(hipEventRecord(S.ev[3], st));
    uint8_t* ho = S.h_out.as<uint8_t>();
    const size_t tail = (size_t)n * (sizeof(slideo_verdict) + sizeof(FrameCands));
    HIP_CHECK(hipMemcpyAsync(ho, S.d_verdicts.p, (size_t)n * sizeof(slideo_verdict), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(ho + (size_t)n * sizeof(slideo_verdict), S.d_fcs.p, (size_t)n * sizeof(FrameCands), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(ho + tail, flags, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(ho + tail + 4, S.d_info.p, 8, hipMemcpyDeviceToHost, st));      // {Qtot, max keypoints per frame}
    if (prof) HIP_CHECK(hipEventRecord(S.ev[4], st));
    S.busy = true; S.n = n;
}

// launch attributes of the stage's kernels (slideo_matcher_create)
void verify_stage_init(slideo_matcher* m) {
    (void)m;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&vote_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_kernel<RANSAC_SMALL_PTS, 0, 0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_lds_bytes(RANSAC_SMALL_PTS, 0)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1, 0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_lds_bytes(RANSAC_LDS_PTS, 0)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_kernel<RANSAC_SMALL_PTS, 0, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_lds_bytes(RANSAC_SMALL_PTS, 1)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_lds_bytes(RANSAC_LDS_PTS, 1)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_kernel<RANSAC_SMALL_PTS, 0, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_lds_bytes(RANSAC_SMALL_PTS, 2)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_kernel<RANSAC_LDS_PTS, RANSAC_SMALL_PTS + 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_lds_bytes(RANSAC_LDS_PTS, 2)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&refine_h_eigen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)refine_h_eigen_lds_bytes()));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_tail_kernel<1, RANSAC_H_TAIL_WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_tail_lds_bytes(RANSAC_H_TAIL_WAVES)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_tail_kernel<2, RANSAC_H_TAIL_WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ransac_h_tail_lds_bytes(RANSAC_H_TAIL_WAVES)));
}

}  // namespace slideo

// ---- Match evidence map (include/slideo_amd.h "Match evidence map") ------------------------------------------------------------------
extern "C" {

int32_t slideo_matcher_evidence_begin(slideo_matcher* m, int32_t cell, int32_t min_inliers) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!evidence_cell_ok(cell)) fail(SLIDEO_ERR_INVALID_ARG, "evidence_begin: cell %d is none of 16, 32, 64", cell);
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "evidence_begin: min_inliers %d below 0", min_inliers);
    if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "evidence_begin: the evidence map is not defined in SIFT mode");
    require_idle(m);
    if (m->evidence.on) fail(SLIDEO_ERR_STATE, "evidence_begin: a session is open (slideo_matcher_evidence_end first)");
    m->evidence = slideo_matcher::Evidence{};
    m->evidence.on = true; m->evidence.cell = cell; m->evidence.min_inliers = min_inliers;
    m->evidence.max_frames = std::min<int64_t>(EV_MAX_FRAMES, std::max<long>(1, env_long("SLIDEO_EVIDENCE_MAX_FRAMES", EV_MAX_FRAMES)));
    API_CATCH(m)
}

int32_t slideo_matcher_evidence_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    evidence_drop(m);
    m->d_evidence.release();
    API_CATCH(m)
}

int32_t slideo_matcher_evidence_info(slideo_matcher* m, int32_t* cell, int32_t* min_inliers, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                     int64_t* frames_through, int64_t* frames_counted) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!cell || !min_inliers || !aw || !ah || !gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    const slideo_matcher::Evidence& E = m->evidence;
    if (!E.on) fail(SLIDEO_ERR_STATE, "no evidence session: slideo_matcher_evidence_begin first");
    *cell = E.cell; *min_inliers = E.min_inliers; *aw = E.aw; *ah = E.ah; *gw = E.gw; *gh = E.gh;
    *frames_through = E.through; *frames_counted = E.counted;
    API_CATCH(m)
}

int32_t slideo_matcher_evidence_counts(slideo_matcher* m, uint32_t* seen_out, uint32_t* hit_out, int64_t capacity_elems, int32_t* gw, int32_t* gh,
                                       int64_t* frames_through, int64_t* frames_counted) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null gw/gh/frames_through/frames_counted");
    require_idle(m);
    const slideo_matcher::Evidence& E = m->evidence;
    if (!E.on) fail(SLIDEO_ERR_STATE, "no evidence session: slideo_matcher_evidence_begin first");
    *gw = E.gw; *gh = E.gh; *frames_through = E.through; *frames_counted = E.counted;
    if (E.aw == 0 || (!seen_out && !hit_out)) return SLIDEO_OK;      // (no counted call yet: a grid of 0 x 0)
    if (!seen_out || !hit_out) fail(SLIDEO_ERR_INVALID_ARG, "seen_out and hit_out go together");
    const int64_t nc = (int64_t)E.gw * E.gh;
    if (nc > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the counts need %lld elements each", (long long)nc);
    HIP_CHECK(hipSetDevice(m->device));
    HIP_CHECK(hipMemcpyAsync(seen_out, m->d_evidence.p, (size_t)nc * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipMemcpyAsync(hit_out, m->d_evidence.as<uint32_t>() + nc, (size_t)nc * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    API_CATCH(m)
}

static int32_t evidence_grid_check(const uint32_t* seen, const uint32_t* hit, int32_t gw, int32_t gh, int32_t cell, int32_t aw, int32_t ah) {
    if (!seen || !hit || !evidence_cell_ok(cell) || aw < 1 || ah < 1 || aw > MAX_DIM || ah > MAX_DIM) return SLIDEO_ERR_INVALID_ARG;
    if (gw != cdiv(aw, cell) || gh != cdiv(ah, cell)) return SLIDEO_ERR_INVALID_ARG;
    return SLIDEO_OK;
}

int32_t slideo_evidence_mask(const uint32_t* seen, const uint32_t* hit, int32_t gw, int32_t gh, int32_t cell, int32_t aw, int32_t ah, int64_t min_seen,
                             int32_t min_hit_ppm, int32_t grow, uint8_t* mask_out, int64_t stride_bytes) {
    if (evidence_grid_check(seen, hit, gw, gh, cell, aw, ah) != SLIDEO_OK || !mask_out || stride_bytes < aw) return SLIDEO_ERR_INVALID_ARG;
    if (min_seen < 0 || min_seen > 0xFFFFFFFFll || min_hit_ppm < 0 || min_hit_ppm > 1000000 || grow < 0 || grow > 256) return SLIDEO_ERR_INVALID_ARG;
    try { evidence_mask(seen, hit, gw, gh, cell, aw, ah, (uint32_t)min_seen, (uint32_t)min_hit_ppm, grow, mask_out, stride_bytes); }
    catch (const std::bad_alloc&) { return SLIDEO_ERR_CAPACITY; }      // (two bytes per cell of host memory)
    return SLIDEO_OK;
}

int32_t slideo_evidence_box(const uint32_t* seen, const uint32_t* hit, int32_t gw, int32_t gh, int32_t cell, int32_t aw, int32_t ah, int64_t min_hits,
                            int32_t min_hit_ppm, int32_t* box_out4) {
    if (evidence_grid_check(seen, hit, gw, gh, cell, aw, ah) != SLIDEO_OK || !box_out4) return SLIDEO_ERR_INVALID_ARG;
    if (min_hits < 0 || min_hits > 0xFFFFFFFFll || min_hit_ppm < 0 || min_hit_ppm > 1000000) return SLIDEO_ERR_INVALID_ARG;
    evidence_box(seen, hit, gw, gh, cell, aw, ah, (uint32_t)min_hits, (uint32_t)min_hit_ppm, box_out4);
    return SLIDEO_OK;
}

}  // extern "C"

// ---- Match tone table (include/slideo_amd.h "Match tone table") ----------------------------------------------------------------------
extern "C" {

int32_t slideo_matcher_tone_begin(slideo_matcher* m, int32_t min_inliers, int32_t min_hits, int32_t flat) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "tone_begin: min_inliers %d below 0", min_inliers);
    if (min_hits < 1) fail(SLIDEO_ERR_INVALID_ARG, "tone_begin: min_hits %d below 1", min_hits);
    if (flat < 0 || flat > 255) fail(SLIDEO_ERR_INVALID_ARG, "tone_begin: flat %d outside 0..255", flat);
    if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "tone_begin: the tone table is not defined in SIFT mode");
    require_idle(m);
    if (m->tone.on) fail(SLIDEO_ERR_STATE, "tone_begin: a session is open (slideo_matcher_tone_end first)");
    HIP_CHECK(hipSetDevice(m->device));
    const size_t bytes = (size_t)(TONE_BINS + 1) * 8;
    m->d_tone.reserve(bytes + 16);
    HIP_CHECK(hipMemsetAsync(m->d_tone.p, 0, bytes, m->stream));      // (the zeroed counts stand before any unit is submitted)
    HIP_CHECK(hipStreamSynchronize(m->stream));
    m->tone = slideo_matcher::Tone{};
    m->tone.on = true; m->tone.min_inliers = min_inliers; m->tone.min_hits = min_hits; m->tone.flat = flat;
    m->tone.max_frames = std::min<int64_t>(TONE_MAX_FRAMES, std::max<long>(1, env_long("SLIDEO_TONE_MAX_FRAMES", (long)TONE_MAX_FRAMES)));
    API_CATCH(m)
}

int32_t slideo_matcher_tone_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    tone_drop(m);
    m->d_tone.release();
    API_CATCH(m)
}

int32_t slideo_matcher_tone_info(slideo_matcher* m, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int64_t* frames_through) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!min_inliers || !min_hits || !flat || !frames_through) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    const slideo_matcher::Tone& T = m->tone;
    if (!T.on) fail(SLIDEO_ERR_STATE, "no tone session: slideo_matcher_tone_begin first");
    *min_inliers = T.min_inliers; *min_hits = T.min_hits; *flat = T.flat; *frames_through = T.through;
    API_CATCH(m)
}

int32_t slideo_matcher_tone_counts(slideo_matcher* m, uint64_t* cnt_out, uint64_t* sum_out, int64_t* frames_through, int64_t* frames_counted) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!cnt_out || !sum_out || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null cnt_out/sum_out/frames_through/frames_counted");
    require_idle(m);
    const slideo_matcher::Tone& T = m->tone;
    if (!T.on) fail(SLIDEO_ERR_STATE, "no tone session: slideo_matcher_tone_begin first");
    HIP_CHECK(hipSetDevice(m->device));
    uint64_t counted = 0;
    HIP_CHECK(hipMemcpyAsync(cnt_out, m->d_tone.p, 768 * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipMemcpyAsync(sum_out, m->d_tone.as<uint64_t>() + 768, 768 * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipMemcpyAsync(&counted, m->d_tone.as<uint64_t>() + TONE_BINS, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    *frames_through = T.through; *frames_counted = (int64_t)counted;
    API_CATCH(m)
}

int32_t slideo_tone_lut(const uint64_t* cnt, const uint64_t* sum, int64_t min_count, uint8_t* lut_out) {
    if (!cnt || !sum || !lut_out || min_count < 1) return SLIDEO_ERR_INVALID_ARG;
    // (no mean above 255, and 2 * sum + cnt stays far inside u64)
    for (int i = 0; i < 768; ++i)
        if (cnt[i] > ((uint64_t)1 << 48) || sum[i] > 255 * cnt[i]) return SLIDEO_ERR_INVALID_ARG;
    return tone_lut(cnt, sum, (uint64_t)min_count, lut_out) ? SLIDEO_OK : SLIDEO_ERR_INVALID_ARG;
}

}  // extern "C"

// ---- Match placement map (include/slideo_amd.h "Match placement map") ---------------------------------------------------------------
extern "C" {

int32_t slideo_matcher_placement_begin(slideo_matcher* m, int32_t cell, int32_t min_inliers, double reach) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!evidence_cell_ok(cell)) fail(SLIDEO_ERR_INVALID_ARG, "placement_begin: cell %d is none of 16, 32, 64", cell);
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "placement_begin: min_inliers %d below 0", min_inliers);
    if (!(reach > 0.0) || !std::isfinite(reach * reach)) fail(SLIDEO_ERR_INVALID_ARG, "placement_begin: reach %g is not a finite distance above 0", reach);
    if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "placement_begin: the placement map is not defined in SIFT mode");
    require_idle(m);
    if (m->placement.on) fail(SLIDEO_ERR_STATE, "placement_begin: a session is open (slideo_matcher_placement_end first)");
    m->placement = slideo_matcher::Placement{};
    m->placement.on = true; m->placement.cell = cell; m->placement.min_inliers = min_inliers; m->placement.reach = reach;
    m->placement.max_frames = std::min<int64_t>(PL_MAX_FRAMES, std::max<long>(1, env_long("SLIDEO_PLACEMENT_MAX_FRAMES", (long)PL_MAX_FRAMES)));
    API_CATCH(m)
}

int32_t slideo_matcher_placement_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    placement_drop(m);
    m->d_placement.release();
    API_CATCH(m)
}

int32_t slideo_matcher_placement_info(slideo_matcher* m, int32_t* cell, int32_t* min_inliers, double* reach, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                      int64_t* frames_through) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!cell || !min_inliers || !reach || !aw || !ah || !gw || !gh || !frames_through) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    const slideo_matcher::Placement& P = m->placement;
    if (!P.on) fail(SLIDEO_ERR_STATE, "no placement session: slideo_matcher_placement_begin first");
    *cell = P.cell; *min_inliers = P.min_inliers; *reach = P.reach; *aw = P.aw; *ah = P.ah; *gw = P.gw; *gh = P.gh; *frames_through = P.through;
    API_CATCH(m)
}

int32_t slideo_matcher_placement_sums(slideo_matcher* m, uint64_t* n_out, uint64_t* sfx_out, uint64_t* sfy_out, uint64_t* su_out, uint64_t* sv_out,
                                      int64_t capacity_elems, int32_t* gw, int32_t* gh, int64_t* frames_through, int64_t* frames_counted) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null gw/gh/frames_through/frames_counted");
    require_idle(m);
    const slideo_matcher::Placement& P = m->placement;
    if (!P.on) fail(SLIDEO_ERR_STATE, "no placement session: slideo_matcher_placement_begin first");
    *gw = P.gw; *gh = P.gh; *frames_through = P.through; *frames_counted = 0;
    if (P.aw == 0) return SLIDEO_OK;      // (no counted call yet: a grid of 0 x 0)
    uint64_t* outs[5] = {n_out, sfx_out, sfy_out, su_out, sv_out};
    int given = 0;
    for (uint64_t* o : outs) given += o != nullptr;
    if (given != 0 && given != 5) fail(SLIDEO_ERR_INVALID_ARG, "the five output arrays go together");
    const int64_t nc = (int64_t)P.gw * P.gh;
    if (given && nc > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the sums need %lld elements each", (long long)nc);
    HIP_CHECK(hipSetDevice(m->device));
    uint64_t counted = 0;
    for (int i = 0; given && i < 5; ++i)
        HIP_CHECK(hipMemcpyAsync(outs[i], m->d_placement.as<uint64_t>() + (size_t)i * nc, (size_t)nc * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipMemcpyAsync(&counted, m->d_placement.as<uint64_t>() + 5 * (size_t)nc, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    *frames_counted = (int64_t)counted;
    API_CATCH(m)
}

int32_t slideo_placement_quad(const uint64_t* n, const uint64_t* sfx, const uint64_t* sfy, const uint64_t* su, const uint64_t* sv, int32_t gw, int32_t gh,
                              int32_t cell, int32_t aw, int32_t ah, int64_t min_count, double trim_px, int32_t rounds, double* quad_out8, double* H_out9,
                              int32_t* cells_used, double* rms_px) {
    if (!n || !sfx || !sfy || !su || !sv || !quad_out8 || !H_out9 || !cells_used || !rms_px) return SLIDEO_ERR_INVALID_ARG;
    if (!evidence_cell_ok(cell) || aw < 1 || ah < 1 || aw > MAX_DIM || ah > MAX_DIM || gw != cdiv(aw, cell) || gh != cdiv(ah, cell)) return SLIDEO_ERR_INVALID_ARG;
    if (min_count < 1 || !(trim_px > 0.0) || !std::isfinite(trim_px) || rounds < 0 || rounds > 8) return SLIDEO_ERR_INVALID_ARG;
    // (no session gives a count above 2^32 or a sum above its count times the coordinate's range; the means stay exact in f64)
    for (size_t c = 0; c < (size_t)gw * gh; ++c)
        if (n[c] > ((uint64_t)1 << 32) || sfx[c] > n[c] * 65536 || sfy[c] > n[c] * 65536 || su[c] > n[c] * 1048576 || sv[c] > n[c] * 1048576)
            return SLIDEO_ERR_INVALID_ARG;
    try {
        return placement_quad(n, sfx, sfy, su, sv, gw, gh, aw, ah, (uint64_t)min_count, trim_px, rounds, quad_out8, H_out9, cells_used, rms_px) ? SLIDEO_OK
                                                                                                                                               : SLIDEO_ERR_INVALID_ARG;
    } catch (const std::bad_alloc&) { return SLIDEO_ERR_CAPACITY; }
}

// "Placement lens": the joint fit of lens and quad to the same sums (placement_lens.h)
int32_t slideo_placement_lens(const uint64_t* n, const uint64_t* sfx, const uint64_t* sfy, const uint64_t* su, const uint64_t* sv, int32_t gw, int32_t gh,
                              int32_t cell, int32_t aw, int32_t ah, int64_t min_count, double cx, double cy, double f, int32_t order, double trim_px,
                              int32_t rounds, int32_t iters, double* k_out2, double* quad_out8, double* H_out9, int32_t* cells_used, double* rms_px) {
    if (!n || !sfx || !sfy || !su || !sv || !k_out2 || !quad_out8 || !H_out9 || !cells_used || !rms_px) return SLIDEO_ERR_INVALID_ARG;
    if (!evidence_cell_ok(cell) || aw < 1 || ah < 1 || aw > MAX_DIM || ah > MAX_DIM || gw != cdiv(aw, cell) || gh != cdiv(ah, cell)) return SLIDEO_ERR_INVALID_ARG;
    if (min_count < 1 || !(trim_px > 0.0) || !std::isfinite(trim_px) || rounds < 0 || rounds > 8) return SLIDEO_ERR_INVALID_ARG;
    if (!std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(f) || !(f > 0.0) || !std::isfinite(1.0 / (f * f)) || !(1.0 / (f * f) > 0.0))
        return SLIDEO_ERR_INVALID_ARG;
    if ((order != 1 && order != 2) || iters < 1 || iters > 1000) return SLIDEO_ERR_INVALID_ARG;
    for (size_t c = 0; c < (size_t)gw * gh; ++c)
        if (n[c] > ((uint64_t)1 << 32) || sfx[c] > n[c] * 65536 || sfy[c] > n[c] * 65536 || su[c] > n[c] * 1048576 || sv[c] > n[c] * 1048576)
            return SLIDEO_ERR_INVALID_ARG;
    try {
        return placement_lens(n, sfx, sfy, su, sv, gw, gh, aw, ah, (uint64_t)min_count, cx, cy, f, order, trim_px, rounds, iters, k_out2, quad_out8, H_out9,
                              cells_used, rms_px) ? SLIDEO_OK : SLIDEO_ERR_INVALID_ARG;
    } catch (const std::bad_alloc&) { return SLIDEO_ERR_CAPACITY; }
}

}  // extern "C"

// ---- Match shading map (include/slideo_amd.h "Match shading map") -------------------------------------------------------------------
extern "C" {

int32_t slideo_matcher_shading_begin(slideo_matcher* m, int32_t cell, int32_t min_inliers, int32_t min_hits, int32_t flat) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    shading_map_begin_check(m, cell, min_inliers, min_hits, flat);
    m->shading_map = slideo_matcher::ShadingMap{};
    m->shading_map.on = true; m->shading_map.cell = cell; m->shading_map.min_inliers = min_inliers; m->shading_map.min_hits = min_hits;
    m->shading_map.flat = flat;
    m->shading_map.max_frames = std::min<int64_t>(SHM_MAX_FRAMES, std::max<long>(1, env_long("SLIDEO_SHADING_MAX_FRAMES", (long)SHM_MAX_FRAMES)));
    API_CATCH(m)
}

int32_t slideo_matcher_shading_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    shading_map_drop(m);
    m->d_shading_map.release();
    API_CATCH(m)
}

int32_t slideo_matcher_shading_info(slideo_matcher* m, int32_t* cell, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int32_t* aw, int32_t* ah,
                                    int32_t* gw, int32_t* gh, int64_t* frames_through) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!cell || !min_inliers || !min_hits || !flat || !aw || !ah || !gw || !gh || !frames_through) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    const slideo_matcher::ShadingMap& H = m->shading_map;
    if (!H.on) fail(SLIDEO_ERR_STATE, "no shading session: slideo_matcher_shading_begin first");
    *cell = H.cell; *min_inliers = H.min_inliers; *min_hits = H.min_hits; *flat = H.flat; *aw = H.aw; *ah = H.ah; *gw = H.gw; *gh = H.gh;
    *frames_through = H.through;
    API_CATCH(m)
}

int32_t slideo_matcher_shading_sums(slideo_matcher* m, uint64_t* cnt_out, uint64_t* sum_f_out, uint64_t* sum_p_out, int64_t capacity_elems, int32_t* gw,
                                    int32_t* gh, int64_t* frames_through, int64_t* frames_counted) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null gw/gh/frames_through/frames_counted");
    require_idle(m);
    const slideo_matcher::ShadingMap& H = m->shading_map;
    if (!H.on) fail(SLIDEO_ERR_STATE, "no shading session: slideo_matcher_shading_begin first");
    *gw = H.gw; *gh = H.gh; *frames_through = H.through; *frames_counted = 0;
    if (H.aw == 0) return SLIDEO_OK;      // (no counted call yet: a grid of 0 x 0)
    uint64_t* outs[3] = {cnt_out, sum_f_out, sum_p_out};
    int given = 0;
    for (uint64_t* o : outs) given += o != nullptr;
    if (given != 0 && given != 3) fail(SLIDEO_ERR_INVALID_ARG, "the three output arrays go together");
    const int64_t nc = (int64_t)H.gw * H.gh;
    if (given && nc > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the sums need %lld elements each", (long long)nc);
    HIP_CHECK(hipSetDevice(m->device));
    uint64_t counted = 0;
    for (int i = 0; given && i < 3; ++i)
        HIP_CHECK(hipMemcpyAsync(outs[i], m->d_shading_map.as<uint64_t>() + (size_t)i * nc, (size_t)nc * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipMemcpyAsync(&counted, m->d_shading_map.as<uint64_t>() + 3 * (size_t)nc, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    *frames_counted = (int64_t)counted;
    API_CATCH(m)
}

}  // extern "C"
