// stage_gate_anchor.hip — the gate reference SLIDEO_GATE_ANCHOR of include/slideo_amd.h "Gate reference", with and without the gate
// settle of "Gate settle": a gated unit's pair table, carried SSDs, walk and new state (stage_gate.hip's gate_unit_submit drives
// it), the two settings and the three taps (kernels: gate_anchor.hip.h).  Plain ANCHOR is the settle with a cap of 0 and no
// previous-frame state.  The centred operand and the pair table are the SSD-table engine's (stage_ssd_table.hip), as the direct
// page look-up's are; a unit that also looks pages up builds the operand twice, each into its own workspace: the look-up's is made
// inside direct_unit_lookup, behind the write of the gate state.
#include "runtime.hpp"
#include "gate_anchor.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

namespace {

// S.d_ga_rec: {|a'|^2 n x i64 | SSDs against the carried anchor n x u64, frame 0 against the carried previous frame u64 (under a
// settle) | the unit's last anchor i32 | the deferral count behind the unit u32}
long long* ga_norm(Slot& S) { return S.d_ga_rec.as<long long>(); }
unsigned long long* ga_carried(Slot& S, int n) { return S.d_ga_rec.as<unsigned long long>() + n; }
int32_t* ga_anchor(Slot& S, int n) { return reinterpret_cast<int32_t*>(ga_carried(S, n) + (size_t)n + 1); }
uint32_t* ga_count(Slot& S, int n) { return reinterpret_cast<uint32_t*>(ga_anchor(S, n) + 1); }

// out[0 .. pairs) = the carried SSDs of gate_carried_ssd_kernel, zeroed and summed on st: pairs = n + 1 with a previous frame, n
// with prev null.  Every pair's L bytes are cut across `chunks` blocks so that the chip (256 CUs) is covered by about two blocks
// per CU at n = 1 as at n = 256, a block keeping at least one dword per thread.
void launch_carried_ssd(const uint8_t* weights, const uint8_t* anchor, const uint8_t* prev, const uint8_t* small, int64_t L, int n,
                        unsigned long long* out, hipStream_t st) {
    const int64_t pairs = (int64_t)n + (prev ? 1 : 0);
    HIP_CHECK(hipMemsetAsync(out, 0, (size_t)pairs * 8, st));
    const int64_t body = L / 4 > 0 ? L / 4 - 1 : 0;
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(cdiv64(512, pairs), cdiv64(body, CARRIED_SSD_BLOCK)));
    const dim3 grid((unsigned)chunks, (unsigned)pairs);
    if (weights) gate_carried_ssd_kernel<true><<<grid, CARRIED_SSD_BLOCK, 0, st>>>(anchor, prev, small, L, n, weights, out);
    else gate_carried_ssd_kernel<false><<<grid, CARRIED_SSD_BLOCK, 0, st>>>(anchor, prev, small, L, n, nullptr, out);
    check_launch("gate_carried_ssd_kernel");
}

}  // namespace

// operand, norms and the table dot[i * n + j], i < j, of the n small images at `small` (stride sb = L bytes), on st
void gram_launch(Slot& S, const uint8_t* weights, const uint8_t* small, int64_t L, int n, hipStream_t st) {
    const int64_t kp = ssd_kp(L);
    ssd_operand_build(small, L, nullptr, n, ssd_rows_pad(n), L, kp, S.d_ga_a.as<uint4>(), ga_norm(S), st, weights);
    ssd_table_dots(S.d_ga_a.as<uint4>(), n, nullptr, n, kp, S.d_ga_dot.as<unsigned long long>(), st);
}

void gate_anchor_reserve(slideo_matcher* m, Slot& S, int n, int sw, int sh, bool settle) {
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT) fail(SLIDEO_ERR_CAPACITY, "a gated unit under SLIDEO_GATE_ANCHOR holds at most %d frames (%d)", GATE_ANCHOR_MAX_UNIT, n);
    const int64_t kp = ssd_kp((int64_t)sw * sh * 3);
    S.d_ga_a.reserve((size_t)ssd_rows_pad(n) * (size_t)kp);
    S.d_ga_rec.reserve((size_t)n * 16 + 16);
    S.d_ga_dot.reserve((size_t)n * n * 8);
    if (!settle) return;
    m->d_gate_prev.reserve((size_t)sw * sh * 3);        // (grow only from the state "none", as d_gate_small: no gated unit is reading them)
    m->d_gate_d.reserve(16);
}

void gate_settle_state_from_anchor(slideo_matcher* m, size_t sb, hipStream_t st) {
    m->d_gate_prev.reserve(sb);
    m->d_gate_d.reserve(16);
    HIP_CHECK(hipMemcpyAsync(m->d_gate_prev.p, m->d_gate_small.p, sb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemsetAsync(m->d_gate_d.p, 0, 4, st));
}

void gate_anchor_unit(slideo_matcher* m, Slot& S, const uint8_t* weights, const uint8_t* small, int64_t sb, int n, long long thr, long long thr_s,
                      int32_t max_defer, bool force0, hipEvent_t wait, const GateAnchorOut& out) {
    hipStream_t st = S.st;
    // without a settle: no previous-frame image and no count in the state, nothing of them is read or written
    const bool settle = m->fs.settle_similarity > 0.f;
    uint8_t* prev = settle ? m->d_gate_prev.as<uint8_t>() : nullptr;
    uint32_t* d_state = settle ? m->d_gate_d.as<uint32_t>() : nullptr;
    // every pair of the unit — the sub-diagonal holds each frame against the frame before it —: nothing here reads the gate state
    gram_launch(S, weights, small, sb, n, st);
    // the carried anchor against the unit's frames and, under a settle, the carried previous frame against frame 0, behind the
    // previous gated unit's write of the state
    if (wait) HIP_CHECK(hipStreamWaitEvent(st, wait, 0));
    gate_chain_receive(m, st);                      // (a chained group call's later member: the predecessor's state arrives here)
    if (!force0) launch_carried_ssd(weights, m->d_gate_small.as<uint8_t>(), prev, small, sb, n, ga_carried(S, n), st);
    gate_settle_kernel<<<1, 64, 0, st>>>(S.d_ga_dot.as<unsigned long long>(), ga_norm(S), ga_carried(S, n), n, thr, thr_s, (uint32_t)max_defer, d_state,
                                          force0 ? 1 : 0, out.flags, out.idx, out.count, out.h_head, out.h_ssd, out.h_idx, out.h_flag, ga_anchor(S, n),
                                          ga_count(S, n));
    check_launch("gate_settle_kernel");
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, cdiv64(sb / 4, ANCHOR_STATE_BLOCK * 4)));
    gate_settle_state_kernel<<<blocks, ANCHOR_STATE_BLOCK, 0, st>>>(small, sb, n, ga_anchor(S, n), ga_count(S, n), sb, m->d_gate_small.as<uint8_t>(), prev,
                                                                    d_state);
    check_launch("gate_settle_state_kernel");
}

}  // namespace slideo

extern "C" {

int32_t slideo_matcher_set_gate_reference(slideo_matcher* m, uint32_t ref) {
    return matcher_set(m, SET_GATE_REFERENCE, [&](const FrameSettings& s) { return propose_gate_reference(s, ref); });
}

int32_t slideo_matcher_gate_reference(const slideo_matcher* m, uint32_t* ref) {
    if (!m || !ref) return SLIDEO_ERR_INVALID_ARG;
    *ref = m->fs.gate_ref;
    return SLIDEO_OK;
}

int32_t slideo_small_gram_ssd(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, int32_t use_valid, uint64_t* ssd_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (n < 0 || n > GATE_ANCHOR_MAX_UNIT || sw < 1 || sh < 1 || (int64_t)sw * sh > m->cfg.small_area || (n > 0 && (!small || !ssd_out)))
        fail(SLIDEO_ERR_INVALID_ARG, "small_gram_ssd: %d small images (at most %d) of %dx%d (at most small_area = %d pixels), small and ssd_out not null", n,
             GATE_ANCHOR_MAX_UNIT, sw, sh, m->cfg.small_area);
    const uint8_t* weights = tap_valid_weights(m, "small_gram_ssd", use_valid != 0, sw, sh);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    if (n == 0) return SLIDEO_OK;
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    const size_t sb = (size_t)sw * sh * 3;
    DevBuf d_small;
    d_small.reserve(sb * n + 16);
    gate_anchor_reserve(m, S, n, sw, sh, false);
    HIP_CHECK(hipMemcpyAsync(d_small.p, small, sb * n, hipMemcpyHostToDevice, st));
    gram_launch(S, weights, d_small.as<uint8_t>(), (int64_t)sb, n, st);
    std::vector<long long> norm((size_t)n);
    std::vector<unsigned long long> dot((size_t)n * n);
    HIP_CHECK(hipMemcpyAsync(norm.data(), ga_norm(S), (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(dot.data(), S.d_ga_dot.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // the table holds i < j alone: the read-out mirrors it, as gate_settle_kernel reads one entry
    for (int i = 0; i < n; ++i) {
        ssd_out[(size_t)i * n + i] = 0;
        for (int j = i + 1; j < n; ++j) {
            const uint64_t s = (uint64_t)(norm[i] + norm[j] - 2ll * (long long)dot[(size_t)i * n + j]);
            ssd_out[(size_t)i * n + j] = s; ssd_out[(size_t)j * n + i] = s;
        }
    }
    API_CATCH(m)
}

int32_t slideo_matcher_set_gate_settle(slideo_matcher* m, float settle_similarity, int32_t max_defer) {
    return matcher_set(m, SET_GATE_REFERENCE, [&](const FrameSettings& s) { return propose_gate_settle(s, settle_similarity, max_defer); });
}

int32_t slideo_matcher_gate_settle(const slideo_matcher* m, float* settle_similarity, int32_t* max_defer) {
    if (!m || !settle_similarity || !max_defer) return SLIDEO_ERR_INVALID_ARG;
    *settle_similarity = m->fs.settle_similarity;
    *max_defer = m->fs.settle_max_defer;
    return SLIDEO_OK;
}

int32_t slideo_small_carried_ssd(slideo_matcher* m, const uint8_t* anchor_small, const uint8_t* prev_small, const uint8_t* small, int32_t n, int32_t sw,
                                 int32_t sh, int32_t use_valid, uint64_t* ssd_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT || sw < 1 || sh < 1 || (int64_t)sw * sh > m->cfg.small_area || !anchor_small || !small || !ssd_out)
        fail(SLIDEO_ERR_INVALID_ARG, "small_carried_ssd: %d small images (1 .. %d) of %dx%d (at most small_area = %d pixels), no null argument", n,
             GATE_ANCHOR_MAX_UNIT, sw, sh, m->cfg.small_area);
    const uint8_t* weights = tap_valid_weights(m, "small_carried_ssd", use_valid != 0, sw, sh);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    hipStream_t st = m->slots[0].st;
    // anchor, previous frame and the n images back to back: with an odd image size every byte alignment occurs; prev_small null:
    // the n pairs alone, as plain ANCHOR launches them (the previous frame's place stays unwritten and unread)
    const size_t pairs = (size_t)n + (prev_small ? 1 : 0);
    const size_t sb = (size_t)sw * sh * 3;
    DevBuf d_img, d_out;
    d_img.reserve(sb * ((size_t)n + 2) + 16);
    d_out.reserve(((size_t)n + 1) * 8);
    uint8_t* p = d_img.as<uint8_t>();
    HIP_CHECK(hipMemcpyAsync(p, anchor_small, sb, hipMemcpyHostToDevice, st));
    if (prev_small) HIP_CHECK(hipMemcpyAsync(p + sb, prev_small, sb, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(p + 2 * sb, small, sb * n, hipMemcpyHostToDevice, st));
    launch_carried_ssd(weights, p, prev_small ? p + sb : nullptr, p + 2 * sb, (int64_t)sb, n, d_out.as<unsigned long long>(), st);
    HIP_CHECK(hipMemcpyAsync(ssd_out, d_out.p, pairs * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    API_CATCH(m)
}

int32_t slideo_gate_settle_walk(slideo_matcher* m, const uint64_t* dot, const int64_t* norm, const uint64_t* carried, int32_t n, int64_t thr_c,
                                int64_t thr_s, int32_t max_defer, int32_t d_in, int32_t none, uint8_t* changed_out, uint64_t* ssd_out,
                                int32_t* anchor_out, int32_t* d_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT || !dot || !norm || !carried || !changed_out || !ssd_out || !anchor_out || !d_out)
        fail(SLIDEO_ERR_INVALID_ARG, "gate_settle_walk: %d frames (1 .. %d), no null argument", n, GATE_ANCHOR_MAX_UNIT);
    if (max_defer < 0 || d_in < 0 || d_in > max_defer)
        fail(SLIDEO_ERR_INVALID_ARG, "gate_settle_walk: 0 <= d_in (%d) <= max_defer (%d)", d_in, max_defer);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    hipStream_t st = m->slots[0].st;
    // {dot n * n u64 | norm n i64 | carried n + 1 u64 | ssd n u64 | kept list n i32, its twin n i32 | anchor, d_in, d_out, count, head 2 | flags n, twin n}
    const size_t N = (size_t)n;
    DevBuf d;
    d.reserve((N * N + 3 * N + 1) * 8 + (2 * N + 6) * 4 + 2 * N + 16);
    unsigned long long* d_dot = d.as<unsigned long long>();
    long long* d_norm = reinterpret_cast<long long*>(d_dot + N * N);
    unsigned long long* d_car = reinterpret_cast<unsigned long long*>(d_norm + N);
    unsigned long long* d_ssd = d_car + N + 1;
    int32_t* d_idx = reinterpret_cast<int32_t*>(d_ssd + N);
    int32_t* d_idx2 = d_idx + N;
    int32_t* d_anchor = d_idx2 + N;
    uint32_t* d_din = reinterpret_cast<uint32_t*>(d_anchor + 1);
    uint32_t* d_dout = d_din + 1;
    uint32_t* d_cnt = d_dout + 1;
    uint32_t* d_head = d_cnt + 1;
    uint8_t* d_flag = reinterpret_cast<uint8_t*>(d_head + 2);
    uint8_t* d_flag2 = d_flag + N;
    const uint32_t din = (uint32_t)d_in;
    HIP_CHECK(hipMemcpyAsync(d_dot, dot, N * N * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_norm, norm, N * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_car, carried, (N + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_din, &din, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));            // (din is a stack variable)
    gate_settle_kernel<<<1, 64, 0, st>>>(d_dot, d_norm, d_car, n, thr_c, thr_s, (uint32_t)max_defer, d_din, none ? 1 : 0, d_flag, d_idx, d_cnt, d_head,
                                          d_ssd, d_idx2, d_flag2, d_anchor, d_dout);
    check_launch("gate_settle_kernel");
    std::vector<uint8_t> flags(2 * N);
    std::vector<int32_t> idx(2 * N);
    uint32_t tail[6];                                // anchor, d_in, d_out, count, head
    HIP_CHECK(hipMemcpyAsync(ssd_out, d_ssd, N * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(flags.data(), d_flag, 2 * N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(idx.data(), d_idx, 2 * N * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(tail, d_anchor, sizeof(tail), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // the kernel writes everything twice (device and pinned record): the twins agree, the kept list is the flagged frames ascending
    const uint32_t cnt = tail[3];
    if (tail[4] != cnt || tail[5] != (uint32_t)n || cnt > (uint32_t)n) fail(SLIDEO_ERR_HIP, "internal: settle walk record %u / %u of %u for %d frames", cnt, tail[4], tail[5], n);
    uint32_t k = 0;
    for (size_t j = 0; j < N; ++j) {
        if (flags[j] > 1 || flags[j] != flags[N + j]) fail(SLIDEO_ERR_HIP, "internal: settle walk flags of frame %d: %d, %d", (int)j, (int)flags[j], (int)flags[N + j]);
        if (flags[j] && (k >= cnt || idx[k] != (int32_t)j || idx[N + k] != (int32_t)j)) fail(SLIDEO_ERR_HIP, "internal: settle walk kept list at frame %d", (int)j);
        k += flags[j];
        changed_out[j] = flags[j];
    }
    if (k != cnt) fail(SLIDEO_ERR_HIP, "internal: settle walk kept %u frames, counted %u", k, cnt);
    *anchor_out = (int32_t)tail[0];
    *d_out = (int32_t)tail[2];
    API_CATCH(m)
}

}  // extern "C"
