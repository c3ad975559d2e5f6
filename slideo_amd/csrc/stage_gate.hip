// stage_gate.hip — the changed-frame gate of include/slideo_amd.h "Changed-frame gate": gated units (small images of all frames, SSDs,
// gate_kernel, gather_frames_kernel in front of the unchanged unit_submit), the gate state and its entry points (kernels: gate.hip.h).
// The frame calls that run gated units are capi_runtime.hip's, beside their plain twins.  Under the gate reference SLIDEO_GATE_ANCHOR
// gate_unit_submit hands the SSDs, the flags and the new state to stage_gate_anchor.hip (include/slideo_amd.h "Gate reference" and, a
// setting of the same unit, "Gate settle").
#include "runtime.hpp"
#include "gate.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

void gate_release(slideo_matcher* m) {
    for (Slot& S : m->slots) if (S.ev_gate) { (void)hipEventDestroy(S.ev_gate); S.ev_gate = nullptr; }
}

int64_t gate_ssd_threshold(float changed_similarity_, int64_t n) {
    const int64_t max_ssd = (int64_t)255 * 255 * 3 * n;
    auto changed = [&](int64_t s) { return changed_similarity((unsigned long long)s, (int)n) < changed_similarity_; };
    if (!changed(max_ssd)) return INT64_MAX;
    if (changed(0)) return 0;
    int64_t lo = 0, hi = max_ssd;                   // changed(lo) false, changed(hi) true; the expression is monotone in the SSD
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (changed(mid)) hi = mid; else lo = mid;
    }
    return hi;
}

// ---- frame mask scope (include/slideo_amd.h "Frame mask scope") ----------------------------------------------------------------
// The validity map: B = the mask binarised and replicated to three channels (mask_bgr_kernel), S = to_small_image(B) through the
// run_small_into every frame of that size goes through, then gate_valid_kernel: weights and n_valid.  Set time; the matcher is idle.
void gate_map_build(slideo_matcher* m, const uint8_t* dmask, int pitch, int w, int h, GateMap& out, DevBuf& out_w) {
    hipStream_t st = m->stream;
    DevBuf d_bgr, d_s, d_n;
    d_bgr.reserve((size_t)w * h * 3);
    mask_bgr_kernel<<<(unsigned)cdiv64((int64_t)w * h, GATE_BLOCK), GATE_BLOCK, 0, st>>>(dmask, pitch, w, h, d_bgr.as<uint8_t>());
    check_launch("mask_bgr_kernel");
    int sw = 0, sh = 0;
    run_small_into(m, DevFrames{d_bgr.as<uint8_t>(), w, h, w * 3, (int64_t)w * h * 3}, 1, d_s, st, &sw, &sh);
    const size_t sb = (size_t)sw * sh * 3;
    out = GateMap{};
    out_w.reserve(sb + 4);
    d_n.reserve(8);
    gate_valid_kernel<<<1, GATE_BLOCK, 0, st>>>(d_s.as<uint8_t>(), sw * sh, out_w.as<uint8_t>(), d_n.as<long long>());
    check_launch("gate_valid_kernel");
    long long nv = -1;
    HIP_CHECK(hipMemcpyAsync(&nv, d_n.p, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (nv < 0 || nv > (long long)sw * sh) fail(SLIDEO_ERR_HIP, "internal: %lld valid pixels of a %dx%d small image", nv, sw, sh);
    if (nv == 0)
        fail(SLIDEO_ERR_INVALID_ARG, "frame mask scope: no pixel of the %dx%d small image of a %dx%d frame is valid under this mask (a small "
             "pixel is valid only where every mask pixel it averages is nonzero): the gate would have nothing to compare", sw, sh, w, h);
    out.on = true; out.sw = sw; out.sh = sh; out.n_valid = nv;
}

const uint8_t* gate_map_for(const slideo_matcher* m, int w, int h, int sw, int sh, int* npx) {
    *npx = sw * sh;
    const FrameMask& k = m->fs.mask;
    if (!m->fs.gate_scope()) return nullptr;
    if (w != k.w || h != k.h)
        fail(SLIDEO_ERR_INVALID_ARG, "frame mask scope: the frames are analysed at %dx%d, the mask the gate ignores regions under is %dx%d "
             "(slideo_matcher_set_frame_mask)", w, h, k.w, k.h);
    const GateMap& g = m->fs.gate_map;      // (set-time state against the call's)
    if (!g.on || g.sw != sw || g.sh != sh) fail(SLIDEO_ERR_HIP, "internal: the gate's validity map is %dx%d (%d), the small images are %dx%d", g.sw, g.sh, (int)g.on, sw, sh);
    *npx = (int)g.n_valid;
    return m->d_gate_w.as<uint8_t>();
}

void launch_gate_ssd(const uint8_t* weights, const uint8_t* a, int64_t a_stride, const uint8_t* b, int64_t b_stride, int64_t bytes,
                     unsigned long long* ssd, int n, hipStream_t st) {
    if (!weights) { launch_ssd(a, a_stride, b, b_stride, bytes, ssd, n, st); return; }
    ssd_masked_kernel<<<n, 256, 0, st>>>(a, a_stride, b, b_stride, bytes, weights, ssd);
    check_launch("ssd_masked_kernel");
}

// The frames of a gated call against the gate state: one size and one format family since the last reset.  Nothing is changed here.
void gate_check(const slideo_matcher::GateState& g, const FrameSrc& src) {
    if (g.seen && (g.w != src.w || g.h != src.h || g.yuv != (src.yuv != nullptr)))
        fail(SLIDEO_ERR_STATE, "gated frames changed from %dx%d %s to %dx%d %s without slideo_matcher_gate_reset", g.w, g.h, g.yuv ? "yuv420" : "bgr8",
             src.w, src.h, src.yuv ? "yuv420" : "bgr8");
    if (g.has && !g.seen && (src.plan.sw != g.sw || src.plan.sh != g.sh))
        fail(SLIDEO_ERR_STATE, "the gate holds a %dx%d small image, these frames' is %dx%d: slideo_matcher_gate_reset first", g.sw, g.sh, src.plan.sw,
             src.plan.sh);
}

// slideo_matcher_gate_reset_from_frame_*: the one frame staged as a gated unit stages its frames (slot 0; plain device BGR is read in
// place), its small image written into the gate state behind the last gated unit's write of it.  What slideo_matcher_gate_reset
// leaves with that small image: the frame's own size and format family are not recorded.
void gate_prime(slideo_matcher* m, FrameSrc src, hipStream_t user_stream) {
    // (a single frame under another pixel format has no stride to check: a BGR frame's own, height * stride_bytes, covers one plane)
    if (!src.yuv && m->fs.pixel_format != SLIDEO_PIXEL_BGR8) src.frame_stride = -1;
    validate_frames(src, m, 1, src.p);             // (a gated call's rules; the frame itself stands for the null frames / verdicts check)
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    if (!S.ev_gate) HIP_CHECK(hipEventCreateWithFlags(&S.ev_gate, hipEventDisableTiming));
    if (src.on_device && user_stream) {             // the frame was produced on the caller's stream
        HIP_CHECK(hipEventRecord(S.ev_in, user_stream));
        HIP_CHECK(hipStreamWaitEvent(st, S.ev_in, 0));
    }
    if (m->last_gate_ev && m->last_gate_ev != S.ev_gate) HIP_CHECK(hipStreamWaitEvent(st, m->last_gate_ev, 0));
    const DevFrames f = stage_frames(m, S, src, 0, 1, nullptr, &S.d_gstage);
    run_small_into(m, f, 1, m->d_gate_small, st);
    // under a gate settle the frame is the anchor and the previous frame, nothing deferred
    if (m->fs.settle_similarity > 0.f) gate_settle_state_from_anchor(m, (size_t)src.plan.sw * src.plan.sh * 3, st);
    // with a gate memory the frame is the ring's one entry ("Gate memory")
    if (m->fs.gate_memory > 0) gate_memory_state_from_anchor(m, (size_t)src.plan.sw * src.plan.sh * 3, st);
    HIP_CHECK(hipEventRecord(S.ev_gate, st));
    m->last_gate_ev = S.ev_gate;
    HIP_CHECK(hipStreamSynchronize(st));            // (the caller's frame is free again)
    gate_state_reset(m);
    m->gate.has = true; m->gate.sw = src.plan.sw; m->gate.sh = src.plan.sh;
}

void gate_state_read(slideo_matcher* m, hipEvent_t behind, size_t sb, uint8_t* anchor, uint8_t* prev, uint32_t* d) {
    hipStream_t st = m->copy_st;
    const bool settle = m->fs.settle_similarity > 0.f;
    if (behind) HIP_CHECK(hipStreamWaitEvent(st, behind, 0));
    HIP_CHECK(hipMemcpyAsync(anchor, m->d_gate_small.p, sb, hipMemcpyDeviceToHost, st));
    if (settle) {
        HIP_CHECK(hipMemcpyAsync(prev, m->d_gate_prev.p, sb, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(d, m->d_gate_d.p, 4, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

void gate_state_write(slideo_matcher* m, size_t sb, const uint8_t* anchor, const uint8_t* prev, const uint32_t* d, hipStream_t st) {
    const bool settle = m->fs.settle_similarity > 0.f;
    m->d_gate_small.reserve(sb);                    // (every allocation in front of the first write of the state)
    if (settle) { m->d_gate_prev.reserve(sb); m->d_gate_d.reserve(16); }
    HIP_CHECK(hipMemcpyAsync(m->d_gate_small.p, anchor, sb, hipMemcpyHostToDevice, st));
    if (!settle) return;
    HIP_CHECK(hipMemcpyAsync(m->d_gate_prev.p, prev, sb, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m->d_gate_d.p, d, 4, hipMemcpyHostToDevice, st));
}

// One gated unit: frames [first, first + n) of src through the gate, the changed ones through unit_submit.  One short host wait
// in the middle (the kept count), as the exact-size path's orb_wait_info: the other slots' units keep the GPU busy meanwhile.
void gate_unit_submit(slideo_matcher* m, Slot& S, const FrameSrc& src, int first, int n, hipStream_t cs) {
    hipStream_t st = S.st;
    if (!S.ev_gate) HIP_CHECK(hipEventCreateWithFlags(&S.ev_gate, hipEventDisableTiming));
    // under a direct similarity: the page operand, the set's eligible list and the look-up's workspaces first, so that a failure
    // there leaves the gate state as it was (include/slideo_amd.h "Direct page look-up")
    const FramePlan& P = src.plan;
    const int sw = P.sw, sh = P.sh, npx = P.npx;
    const uint8_t* weights = P.gate_w;
    const bool look = m->fs.direct_t > 0.f;
    DirectPlan plan;
    // the direct scope VALID: over the pixels the gate compares (null without a map in force: whole images)
    if (look) plan = direct_unit_prepare(m, S, n, sw, sh, m->fs.direct_scope == SLIDEO_DIRECT_VALID ? weights : nullptr);
    // under SLIDEO_GATE_ANCHOR: the pair table's workspaces, first for the same reason (include/slideo_amd.h "Gate reference")
    const bool anchor = m->fs.gate_ref == SLIDEO_GATE_ANCHOR;
    // ... under a gate settle also the state's previous-frame image and count ("Gate settle")
    const bool settle = anchor && m->fs.settle_similarity > 0.f;
    // ... with a gate memory also the ring and the unit's table against it ("Gate memory")
    if (anchor) gate_anchor_reserve(m, S, n, sw, sh, settle, m->fs.gate_memory);
    const DevFrames all = stage_frames(m, S, src, first, n, cs, &S.d_gstage);
    run_small_into(m, all, n, S.d_gsmall, st);
    const int64_t sb = (int64_t)sw * sh * 3;
    const uint8_t* small = S.d_gsmall.as<uint8_t>();
    S.d_gate.reserve((size_t)n * 13 + 16);
    unsigned long long* ssd = S.d_gate.as<unsigned long long>();
    int32_t* idx = reinterpret_cast<int32_t*>(S.d_gate.as<uint8_t>() + (size_t)n * 8);
    uint32_t* count = reinterpret_cast<uint32_t*>(idx + n);
    uint8_t* flags = reinterpret_cast<uint8_t*>(count + 1);
    // under a direct similarity the record grows by the look-up's tail (include/slideo_amd.h "Direct page look-up")
    const size_t direct_ofs = (gate_rec_bytes(n) + 7) & ~(size_t)7;
    S.h_gate.reserve(look ? direct_ofs + direct_unit_rec_bytes(n) : gate_rec_bytes(n));
    const bool force0 = !m->gate.has;
    m->d_gate_small.reserve((size_t)sb);            // (grows only from the state "none": no gated unit is reading it)
    const long long thr = gate_ssd_threshold(m->cfg.changed_similarity, npx);
    uint8_t* const hrec = S.h_gate.as<uint8_t>();
    if (anchor) {
        // every pair of the unit, the carried anchor against its frames behind the previous gated unit's write of the state, the walk
        // (gate_kernel's outputs) and the new state: the unit's last flagged frame, if any; without a settle the walk's cap is 0
        const GateAnchorOut out{flags, idx, count, reinterpret_cast<uint32_t*>(hrec), reinterpret_cast<unsigned long long*>(hrec + gate_rec_ssd_ofs()),
                                reinterpret_cast<int32_t*>(hrec + gate_rec_idx_ofs(n)), hrec + gate_rec_flag_ofs(n)};
        hipEvent_t wait = m->last_gate_ev != S.ev_gate ? m->last_gate_ev : nullptr;
        gate_anchor_unit(m, S, weights, small, sb, n, thr, settle ? gate_ssd_threshold(m->fs.settle_similarity, npx) : 0,
                         settle ? m->fs.settle_max_defer : 0, force0, wait, out);
    } else {
        // pair i: (small[i - 1], small[i]); pair 0: (gate state, small[0]), behind the previous gated unit's write of the state
        if (n > 1) launch_gate_ssd(weights, small, sb, small + sb, sb, sb, ssd + 1, n - 1, st);
        if (m->last_gate_ev && m->last_gate_ev != S.ev_gate) HIP_CHECK(hipStreamWaitEvent(st, m->last_gate_ev, 0));
        gate_chain_receive(m, st);                  // (a chained group call's later member: the predecessor's state arrives here)
        if (!force0) launch_gate_ssd(weights, m->d_gate_small.as<uint8_t>(), 0, small, 0, sb, ssd, 1, st);
        HIP_CHECK(hipMemcpyAsync(m->d_gate_small.p, small + sb * (n - 1), (size_t)sb, hipMemcpyDeviceToDevice, st));
    }
    HIP_CHECK(hipEventRecord(S.ev_gate, st));
    m->last_gate_ev = S.ev_gate;
    slideo_matcher::GateState& g = m->gate;
    const int64_t t0 = g.next_ord;                  // (gate_anchor_unit read it: the unit's frames have the ordinals t0 .. t0 + n - 1)
    g.has = true; g.seen = true; g.w = src.w; g.h = src.h; g.yuv = src.yuv != nullptr; g.sw = sw; g.sh = sh; g.next_ord = t0 + n;

    // the look-up of all n frames (it does not depend on the flags); none when no page of the selected set shares the small size
    const bool direct = plan.cls != nullptr;
    if (direct) direct_unit_lookup(S, plan, n);
    if (!anchor) {
        gate_kernel<<<1, GATE_BLOCK, 0, st>>>(ssd, n, thr, force0 ? 1 : 0, flags, idx, count, hrec);
        check_launch("gate_kernel");
    }
    // the direct frames leave the kept list: the one host wait below reads the reduced count
    if (direct)
        direct_unit_gate(m, S, n, npx, idx, count, reinterpret_cast<int32_t*>(S.h_gate.as<uint8_t>() + gate_rec_idx_ofs(n)),
                         S.h_gate.as<uint8_t>() + direct_ofs);
    HIP_CHECK(hipStreamSynchronize(st));
    const GateHostRec rec = *S.h_gate.as<GateHostRec>();
    if (rec.n != (uint32_t)n || rec.count > (uint32_t)n) fail(SLIDEO_ERR_HIP, "internal: gate record %u of %u for a unit of %d", rec.count, rec.n, n);
    int k = (int)rec.count;
    if (direct) {
        const int kept = (int)direct_rec_kept(S.h_gate.as<uint8_t>() + direct_ofs, n);
        if (kept > k) fail(SLIDEO_ERR_HIP, "internal: %d frames kept behind the look-up, %d changed", kept, k);
        k = kept;
    }
    Slot::GateUnit gu;
    gu.on = true; gu.n = n; gu.k = k; gu.sw = sw; gu.sh = sh; gu.npx = npx; gu.force0 = force0; gu.settle = settle;
    gu.direct = direct; gu.direct_t = m->fs.direct_t; gu.direct_ofs = direct_ofs;
    gu.memory = anchor && m->fs.gate_memory > 0; gu.t0 = t0;
    if (k == 0) {                                   // no frame changed (or every changed one is direct): no pipeline; the collect returns at once
        S.busy = true; S.n = 0; S.u_async = false; S.timed = false;
        S.gate = gu;
        return;
    }
    DevFrames f = all;
    if (k < n) {
        // the kept frames back to back in the slot's d_stage (all kept: the staged images as they are)
        const int row_bytes = all.w * 3;
        const int64_t fb = (int64_t)row_bytes * all.h;
        uint8_t* dst = stage_for_upload(m, S, (size_t)fb * k);
        const bool contiguous = all.stride == row_bytes;
        const int64_t seg_bytes = contiguous ? fb : row_bytes;
        const int nseg = contiguous ? 1 : all.h;
        const int bps = contiguous ? (int)std::min<int64_t>(256, std::max<int64_t>(1, cdiv64(fb / 16, GATHER_BLOCK * 8))) : 1;
        const int gx = contiguous ? bps : std::min(all.h, 128);
        gather_frames_kernel<<<dim3(gx, k), GATHER_BLOCK, 0, st>>>(all.p, all.frame_stride, all.stride, idx, seg_bytes, nseg, bps, dst);
        check_launch("gather_frames_kernel");
        f = DevFrames{dst, all.w, all.h, row_bytes, fb};
    }
    unit_submit(m, S, f, k, P.mask_pyr);
    S.gate = gu;
}

void gate_unit_collect(slideo_matcher* m, Slot& S, uint8_t* changed_out, float* similarity_out, slideo_verdict* verdicts_out) {
    const Slot::GateUnit g = S.gate;
    const uint8_t* rec = S.h_gate.as<uint8_t>();
    std::vector<slideo_verdict> v((size_t)g.k);
    if (g.k > 0) unit_collect(m, S, v.data());      // (an overflowed unit is re-run from its gathered frames, S.u_in: never the gate)
    else S.busy = false;
    S.gate.on = false;
    const uint8_t* flag = rec + gate_rec_flag_ofs(g.n);
    // with a gate memory: the unit's refs, behind the synchronous call's earlier units' or, a collected ticket, alone
    const long long* ref = g.memory ? S.h_gm.as<long long>() : nullptr;
    if (g.memory) {
        if (!m->gate_refs_call) m->gate_refs.clear();
        m->gate_refs.insert(m->gate_refs.end(), ref, ref + g.n);
        m->gate_refs_valid = true;
    }
    int r = 0;
    for (int i = 0; i < g.n; ++i) {
        unsigned long long s;
        std::memcpy(&s, rec + gate_rec_ssd_ofs() + (size_t)i * 8, 8);
        const float sim = (i == 0 && g.force0) ? 0.0f : changed_similarity(s, g.npx);      // video_capture.rs:92
        // (under a gate settle a frame away from its anchor may be deferred: flagged => away, and not away => not flagged)
        const bool away = sim < m->cfg.changed_similarity;
        // (with a gate memory a frame away from its anchor may be recalled or deferred — flag 0 —, which ref tells apart: a matched
        // frame stands behind itself, a frame that is not away behind its anchor, never behind nothing)
        if (g.memory ? flag[i] > 1 || (flag[i] != 0 && (!away || ref[i] != g.t0 + i)) || (!away && ref[i] == SLIDEO_GATE_REF_DEFERRED) ||
                           (flag[i] == 0 && (ref[i] >= g.t0 + i || ref[i] < SLIDEO_GATE_REF_DEFERRED)) ||
                           (!g.settle && ref[i] == SLIDEO_GATE_REF_DEFERRED)
                     : g.settle ? (flag[i] != 0 && !away) || flag[i] > 1 : away != (flag[i] != 0))
            fail(SLIDEO_ERR_HIP, "internal: the gate's flag of frame %d (%d, SSD %llu) is not the host expression's", i, (int)flag[i], s);
        changed_out[i] = flag[i];
        if (similarity_out) similarity_out[i] = sim;
        if (!flag[i]) { verdicts_out[i] = slideo_verdict{-1, 0.0f, 0, 0}; continue; }
        if (g.direct) {
            // a changed frame's look-up: the similarity from the SSD read back, the device's decision against the host expression
            const DirectFrameRec d = direct_rec_frame(rec + g.direct_ofs, g.n, i);
            const float s = changed_similarity(d.ssd, g.npx);
            if (d.page < 0 || (s >= g.direct_t) != d.direct)
                fail(SLIDEO_ERR_HIP, "internal: the look-up's decision for frame %d (%d, page %d, SSD %llu) is not the host expression's", i, (int)d.direct,
                     d.page, d.ssd);
            if (d.direct) { verdicts_out[i] = slideo_verdict{d.page, s, 0, 0}; continue; }
        }
        if (r >= g.k) fail(SLIDEO_ERR_HIP, "internal: more frames through the pipeline than the %d it ran for", g.k);
        verdicts_out[i] = v[(size_t)r++];
    }
    if (r != g.k) fail(SLIDEO_ERR_HIP, "internal: %d frames scattered, the pipeline ran for %d", r, g.k);
}

// the header of m's gate state as a record, d still to be read from the device
static GateRecordHead gate_record_head_of(const slideo_matcher* m) {
    GateRecordHead h;
    h.has = m->gate.has; h.gate_ref = m->fs.gate_ref; h.settle = m->fs.settle_similarity > 0.f;
    if (h.has) { h.sw = m->gate.sw; h.sh = m->gate.sh; }
    return h;
}

}  // namespace slideo

extern "C" {

int64_t slideo_changed_ssd_threshold(float changed_similarity, int32_t small_w, int32_t small_h) {
    if (small_w < 1 || small_h < 1 || (int64_t)small_w * small_h > INT32_MAX) return -1;
    return gate_ssd_threshold(changed_similarity, (int64_t)small_w * small_h);
}

int64_t slideo_changed_ssd_threshold_n(float changed_similarity, int64_t n_pixels) {
    if (n_pixels < 1 || n_pixels > INT32_MAX) return -1;
    return gate_ssd_threshold(changed_similarity, n_pixels);
}

int32_t slideo_matcher_gate_reset(slideo_matcher* m, const uint8_t* prev_small, int32_t small_w, int32_t small_h) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (prev_small && (small_w < 1 || small_h < 1 || (int64_t)small_w * small_h > m->cfg.small_area))
        fail(SLIDEO_ERR_INVALID_ARG, "gate_reset: a %dx%d small image (at most small_area = %d pixels)", small_w, small_h, m->cfg.small_area);
    require_idle(m);
    if (!prev_small) { gate_state_reset(m); return SLIDEO_OK; }
    HIP_CHECK(hipSetDevice(m->device));
    const size_t sb = (size_t)small_w * small_h * 3;
    m->d_gate_small.reserve(sb);
    HIP_CHECK(hipMemcpyAsync(m->d_gate_small.p, prev_small, sb, hipMemcpyHostToDevice, m->stream));
    if (m->fs.settle_similarity > 0.f) gate_settle_state_from_anchor(m, sb, m->stream);      // (anchor = previous = that image, nothing deferred)
    if (m->fs.gate_memory > 0) gate_memory_state_from_anchor(m, sb, m->stream);               // (the ring's one entry, SLIDEO_GATE_REF_RESET)
    HIP_CHECK(hipStreamSynchronize(m->stream));
    gate_state_reset(m);
    m->gate.has = true; m->gate.sw = small_w; m->gate.sh = small_h;
    API_CATCH(m)
}

// a list of one (include/slideo_amd.h "Frame lists")
int32_t slideo_matcher_gate_reset_from_frame_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    const FrameSrc src = FrameSrc::from_list(list, m->fs);
    if (list->n_frames != 1) fail(SLIDEO_ERR_INVALID_ARG, "frame list: the gate is reset from a list of one frame (n_frames %d)", list->n_frames);
    gate_prime(m, src, reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_matcher_gate_reset_from_frame_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height, int32_t stride_bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    gate_prime(m, FrameSrc::image(frame, width, height, stride_bytes), nullptr);
    API_CATCH(m)
}

int32_t slideo_matcher_gate_reset_from_frame_yuv420(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height,
                                                    const slideo_yuv420_layout* layout) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    gate_prime(m, FrameSrc::yuv420(frame, false, width, height, layout, -1), nullptr);
    API_CATCH(m)
}

int32_t slideo_matcher_gate_reset_from_frame_bgr8_dev(slideo_matcher* m, const uint8_t* frame_dev, int32_t width, int32_t height,
                                                      int32_t stride_bytes, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    gate_prime(m, FrameSrc::bgr8(frame_dev, true, width, height, stride_bytes, (int64_t)height * stride_bytes),
               reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_matcher_gate_reset_from_frame_yuv420_dev(slideo_matcher* m, const uint8_t* frame_dev, int32_t width, int32_t height,
                                                        const slideo_yuv420_layout* layout, void* hip_stream) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    gate_prime(m, FrameSrc::yuv420(frame_dev, true, width, height, layout, -1), reinterpret_cast<hipStream_t>(hip_stream));
    API_CATCH(m)
}

int32_t slideo_matcher_gate_last_small(slideo_matcher* m, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!sw || !sh) fail(SLIDEO_ERR_INVALID_ARG, "null sw/sh");
    require_idle(m);
    if (!m->gate.has) fail(SLIDEO_ERR_STATE, "the gate state is \"none\": no frame was gated since the last reset");
    *sw = m->gate.sw; *sh = m->gate.sh;
    const int64_t sb = (int64_t)m->gate.sw * m->gate.sh * 3;
    if (sb > out_capacity) fail(SLIDEO_ERR_CAPACITY, "small image needs %lld bytes", (long long)sb);
    if (out) {
        HIP_CHECK(hipSetDevice(m->device));
        if (m->fs.gate_memory > 0) { gate_memory_read_anchor(m, (size_t)sb, out); return SLIDEO_OK; }      // (the anchor is a slot of the ring)
        for (Slot& S : m->slots) HIP_CHECK(hipStreamSynchronize(S.st));          // (a collected unit's write of the state may still be running)
        HIP_CHECK(hipMemcpyAsync(out, m->d_gate_small.p, (size_t)sb, hipMemcpyDeviceToHost, m->stream));
        HIP_CHECK(hipStreamSynchronize(m->stream));
    }
    API_CATCH(m)
}

// ---- the gate state as a record (include/slideo_amd.h "Gate state record"; the header: frame_settings.h) -----------------------------
int32_t slideo_matcher_gate_state_bytes(slideo_matcher* m, int64_t* bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bytes) fail(SLIDEO_ERR_INVALID_ARG, "null bytes");
    gate_record_memory_rule(m->fs.gate_memory);
    require_idle(m);
    *bytes = gate_record_head_of(m).bytes();
    API_CATCH(m)
}

int32_t slideo_matcher_gate_state_export(slideo_matcher* m, uint8_t* out, int64_t capacity, int64_t* bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!bytes) fail(SLIDEO_ERR_INVALID_ARG, "null bytes");
    gate_record_memory_rule(m->fs.gate_memory);
    require_idle(m);
    GateRecordHead h = gate_record_head_of(m);
    *bytes = h.bytes();
    if (!out || h.bytes() > capacity) fail(SLIDEO_ERR_CAPACITY, "the gate state record needs %lld bytes", (long long)h.bytes());
    if (h.has) {
        HIP_CHECK(hipSetDevice(m->device));
        for (Slot& S : m->slots) HIP_CHECK(hipStreamSynchronize(S.st));          // (a collected unit's write of the state may still be running)
        const size_t sb = (size_t)h.image_bytes();
        gate_state_read(m, m->last_gate_ev, sb, out + GATE_RECORD_HEADER, out + GATE_RECORD_HEADER + sb, &h.d);
    }
    gate_record_encode(h, out);
    API_CATCH(m)
}

int32_t slideo_matcher_gate_state_import(slideo_matcher* m, const uint8_t* rec, int64_t bytes) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    gate_record_memory_rule(m->fs.gate_memory);
    const GateRecordHead h = gate_record_validate(rec, bytes, m->fs.gate_ref, m->fs.settle_similarity, m->fs.settle_max_defer, m->cfg.small_area);
    require_idle(m);
    if (!h.has) { gate_state_reset(m); return SLIDEO_OK; }
    HIP_CHECK(hipSetDevice(m->device));
    const size_t sb = (size_t)h.image_bytes();
    const uint32_t d = h.d;
    if (m->last_gate_ev) HIP_CHECK(hipStreamWaitEvent(m->stream, m->last_gate_ev, 0));
    gate_state_write(m, sb, rec + GATE_RECORD_HEADER, rec + GATE_RECORD_HEADER + sb, &d, m->stream);
    HIP_CHECK(hipStreamSynchronize(m->stream));      // (the record and d are the caller's and this frame's)
    gate_state_reset(m);
    m->gate.has = true; m->gate.sw = h.sw; m->gate.sh = h.sh;
    API_CATCH(m)
}

}  // extern "C"
