// stage_gate_settle.hip — the gate settle of include/slideo_amd.h "Gate settle": under SLIDEO_GATE_ANCHOR a gated unit's carried SSDs,
// walk and new state when a settle is in force (stage_gate.hip's gate_unit_submit drives it), the setting and the taps (kernels:
// gate_settle.hip.h).  The centred operand and the pair table are stage_gate_anchor.hip's gram_launch, as they are.
#include "runtime.hpp"
#include "gate_settle.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

namespace {

// S.d_gs_rec: {SSDs against the carried anchor n x u64, frame 0 against the carried previous frame u64 | last anchor i32 | count u32}
unsigned long long* gs_carried(Slot& S) { return S.d_gs_rec.as<unsigned long long>(); }
int32_t* gs_anchor(Slot& S, int n) { return reinterpret_cast<int32_t*>(S.d_gs_rec.as<unsigned long long>() + (size_t)n + 1); }
uint32_t* gs_count(Slot& S, int n) { return reinterpret_cast<uint32_t*>(gs_anchor(S, n) + 1); }

// out[0 .. n] = the n + 1 carried SSDs of gate_carried_ssd_kernel, zeroed and summed on st.  Every pair's L bytes are cut across
// `chunks` blocks so that the chip (256 CUs) is covered by about two blocks per CU at n = 1 as at n = 256, a block keeping at least
// one dword per thread.
void launch_carried_ssd(const uint8_t* weights, const uint8_t* anchor, const uint8_t* prev, const uint8_t* small, int64_t L, int n,
                        unsigned long long* out, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(out, 0, ((size_t)n + 1) * 8, st));
    const int64_t body = L / 4 > 0 ? L / 4 - 1 : 0;
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(cdiv64(512, (int64_t)n + 1), cdiv64(body, CARRIED_SSD_BLOCK)));
    const dim3 grid((unsigned)chunks, (unsigned)n + 1);
    if (weights) gate_carried_ssd_kernel<true><<<grid, CARRIED_SSD_BLOCK, 0, st>>>(anchor, prev, small, L, n, weights, out);
    else gate_carried_ssd_kernel<false><<<grid, CARRIED_SSD_BLOCK, 0, st>>>(anchor, prev, small, L, n, nullptr, out);
    check_launch("gate_carried_ssd_kernel");
}

}  // namespace

void gate_settle_reserve(slideo_matcher* m, Slot& S, int n, int sw, int sh) {
    gate_anchor_reserve(S, n, sw, sh);
    S.d_gs_rec.reserve(((size_t)n + 1) * 8 + 16);
    m->d_gate_prev.reserve((size_t)sw * sh * 3);        // (grow only from the state "none", as d_gate_small: no gated unit is reading them)
    m->d_gate_d.reserve(16);
}

void gate_settle_state_from_anchor(slideo_matcher* m, size_t sb, hipStream_t st) {
    m->d_gate_prev.reserve(sb);
    m->d_gate_d.reserve(16);
    HIP_CHECK(hipMemcpyAsync(m->d_gate_prev.p, m->d_gate_small.p, sb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemsetAsync(m->d_gate_d.p, 0, 4, st));
}

void gate_settle_unit(slideo_matcher* m, Slot& S, const uint8_t* weights, const uint8_t* small, int64_t sb, int n, long long thr, long long thr_s,
                      bool force0, hipEvent_t wait, const GateAnchorOut& out) {
    hipStream_t st = S.st;
    // every pair of the unit — the sub-diagonal holds each frame against the frame before it —: nothing here reads the gate state
    gram_launch(S, weights, small, sb, n, st);
    // the carried anchor against the unit's frames and the carried previous frame against frame 0, behind the previous gated unit's
    // write of the state
    if (wait) HIP_CHECK(hipStreamWaitEvent(st, wait, 0));
    if (!force0) launch_carried_ssd(weights, m->d_gate_small.as<uint8_t>(), m->d_gate_prev.as<uint8_t>(), small, sb, n, gs_carried(S), st);
    gate_settle_kernel<<<1, 64, 0, st>>>(S.d_ga_dot.as<unsigned long long>(), S.d_ga_rec.as<long long>(), gs_carried(S), n, thr, thr_s,
                                          (uint32_t)m->fs.settle_max_defer, m->d_gate_d.as<uint32_t>(), force0 ? 1 : 0, out.flags, out.idx, out.count,
                                          out.h_head, out.h_ssd, out.h_idx, out.h_flag, gs_anchor(S, n), gs_count(S, n));
    check_launch("gate_settle_kernel");
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, cdiv64(sb / 4, SETTLE_STATE_BLOCK * 4)));
    gate_settle_state_kernel<<<blocks, SETTLE_STATE_BLOCK, 0, st>>>(small, sb, n, gs_anchor(S, n), gs_count(S, n), sb, m->d_gate_small.as<uint8_t>(),
                                                                    m->d_gate_prev.as<uint8_t>(), m->d_gate_d.as<uint32_t>());
    check_launch("gate_settle_state_kernel");
}

}  // namespace slideo

extern "C" {

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
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT || sw < 1 || sh < 1 || (int64_t)sw * sh > m->cfg.small_area || !anchor_small || !prev_small || !small || !ssd_out)
        fail(SLIDEO_ERR_INVALID_ARG, "small_carried_ssd: %d small images (1 .. %d) of %dx%d (at most small_area = %d pixels), no null argument", n,
             GATE_ANCHOR_MAX_UNIT, sw, sh, m->cfg.small_area);
    const uint8_t* weights = tap_valid_weights(m, "small_carried_ssd", use_valid != 0, sw, sh);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    hipStream_t st = m->slots[0].st;
    // anchor, previous frame and the n images back to back: with an odd image size every byte alignment occurs
    const size_t sb = (size_t)sw * sh * 3;
    DevBuf d_img, d_out;
    d_img.reserve(sb * ((size_t)n + 2) + 16);
    d_out.reserve(((size_t)n + 1) * 8);
    uint8_t* p = d_img.as<uint8_t>();
    HIP_CHECK(hipMemcpyAsync(p, anchor_small, sb, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(p + sb, prev_small, sb, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(p + 2 * sb, small, sb * n, hipMemcpyHostToDevice, st));
    launch_carried_ssd(weights, p, p + sb, p + 2 * sb, (int64_t)sb, n, d_out.as<unsigned long long>(), st);
    HIP_CHECK(hipMemcpyAsync(ssd_out, d_out.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
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
