// stage_gate_anchor.hip — the gate reference SLIDEO_GATE_ANCHOR of include/slideo_amd.h "Gate reference", with and without the gate
// settle of "Gate settle": a gated unit's pair table, carried SSDs, walk and new state (stage_gate.hip's gate_unit_submit drives
// it), the two settings and the three taps (kernels: gate_anchor.hip.h).  Plain ANCHOR is the settle with a cap of 0 and no
// previous-frame state.  The centred operand and the pair table are the SSD-table engine's (stage_ssd_table.hip), as the direct
// page look-up's are; a unit that also looks pages up builds the operand twice, each into its own workspace: the look-up's is made
// inside direct_unit_lookup, behind the write of the gate state.  With a gate memory in force ("Gate memory") gate_memory_unit stands
// in gate_anchor_unit's place: the ring of the last M matched frames, its operand and the n x M table in front of gate_recall_kernel,
// gate_memory_state_kernel behind it; the memory's setting, the refs call and its three taps are at the end of this file.
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

// S.d_gm_rec: {|e'|^2 of the ring's slots 64 x i64 | frame 0 against the carried previous frame u64 | the walk's GateMemoryUnit |
// ref n x i64}
constexpr size_t GM_PREV_OFS = (size_t)GATE_MEMORY_SLOTS * 8, GM_UNIT_OFS = GM_PREV_OFS + 8, GM_REF_OFS = GM_UNIT_OFS + sizeof(GateMemoryUnit);
static_assert(GM_REF_OFS % 8 == 0, "the refs are i64");
long long* gm_norm(Slot& S) { return S.d_gm_rec.as<long long>(); }
unsigned long long* gm_prev_ssd(Slot& S) { return reinterpret_cast<unsigned long long*>(S.d_gm_rec.as<uint8_t>() + GM_PREV_OFS); }
GateMemoryUnit* gm_unit(Slot& S) { return reinterpret_cast<GateMemoryUnit*>(S.d_gm_rec.as<uint8_t>() + GM_UNIT_OFS); }
long long* gm_ref(Slot& S) { return reinterpret_cast<long long*>(S.d_gm_rec.as<uint8_t>() + GM_REF_OFS); }
// a slot of the ring: a small image's bytes, padded so that every slot is 16-byte aligned (gate_memory_state_kernel stores dwords)
int64_t gm_slot_bytes(size_t sb) { return (int64_t)((sb + 15) / 16 * 16); }

// the matcher's ring for small images of sb bytes: M slots and the meta (grows only from the state "none")
void gate_memory_reserve_ring(slideo_matcher* m, size_t sb) {
    const int M = m->fs.gate_memory;
    m->d_gm_img.reserve((size_t)gm_slot_bytes(sb) * (size_t)M + 16);
    m->d_gm_meta.reserve(sizeof(GateMemoryMeta));
    m->gm_stride = gm_slot_bytes(sb);
}

// The unit's gate with a memory of M slots in force ("Gate memory"): gate_anchor_unit's steps with the ring in the anchor's place
void gate_memory_unit(slideo_matcher* m, Slot& S, const uint8_t* weights, const uint8_t* small, int64_t sb, int n, long long thr, long long thr_s,
                      int32_t max_defer, bool force0, hipEvent_t wait, const GateAnchorOut& out) {
    hipStream_t st = S.st;
    const int M = m->fs.gate_memory;
    const bool settle = m->fs.settle_similarity > 0.f;
    uint8_t* prev = settle ? m->d_gate_prev.as<uint8_t>() : nullptr;
    const long long t0 = m->gate.next_ord;
    gram_launch(S, weights, small, sb, n, st);
    if (wait) HIP_CHECK(hipStreamWaitEvent(st, wait, 0));
    gate_chain_receive(m, st);                      // (a group of one member never chains: nothing arrives)
    if (!force0) {
        // the ring's whole small images under the weights in force now (a frame-mask change keeps the gate state), every frame
        // against every slot, and frame 0 against the carried previous frame
        const int64_t kp = ssd_kp(sb);
        ssd_operand_build(m->d_gm_img.as<uint8_t>(), m->gm_stride, nullptr, M, ssd_rows_pad(M), sb, kp, S.d_gm_op.as<uint4>(), gm_norm(S), st, weights);
        ssd_table_dots(S.d_ga_a.as<uint4>(), n, S.d_gm_op.as<uint4>(), M, kp, S.d_gm_dot.as<unsigned long long>(), st);
        if (settle) launch_carried_ssd(weights, prev, prev, small, sb, 0, gm_prev_ssd(S), st);
    }
    gate_recall_kernel<<<1, 64, 0, st>>>(S.d_ga_dot.as<unsigned long long>(), ga_norm(S), S.d_gm_dot.as<unsigned long long>(), gm_norm(S),
                                          m->d_gm_meta.as<GateMemoryMeta>(), gm_prev_ssd(S), n, M, t0, thr, thr_s, (uint32_t)max_defer, force0 ? 1 : 0,
                                          out.flags, out.idx, out.count, out.h_head, out.h_ssd, out.h_idx, out.h_flag, gm_ref(S), S.h_gm.as<long long>(),
                                          gm_unit(S));
    check_launch("gate_recall_kernel");
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, cdiv64(sb / 4, ANCHOR_STATE_BLOCK * 4)));
    gate_memory_state_kernel<<<dim3(blocks, (unsigned)(M + (settle ? 1 : 0))), ANCHOR_STATE_BLOCK, 0, st>>>(
        small, sb, n, M, t0, gm_unit(S), sb, m->d_gm_img.as<uint8_t>(), m->gm_stride, prev, m->d_gm_meta.as<GateMemoryMeta>());
    check_launch("gate_memory_state_kernel");
}

}  // namespace

// operand, norms and the table dot[i * n + j], i < j, of the n small images at `small` (stride sb = L bytes), on st
void gram_launch(Slot& S, const uint8_t* weights, const uint8_t* small, int64_t L, int n, hipStream_t st) {
    const int64_t kp = ssd_kp(L);
    ssd_operand_build(small, L, nullptr, n, ssd_rows_pad(n), L, kp, S.d_ga_a.as<uint4>(), ga_norm(S), st, weights);
    ssd_table_dots(S.d_ga_a.as<uint4>(), n, nullptr, n, kp, S.d_ga_dot.as<unsigned long long>(), st);
}

void gate_anchor_reserve(slideo_matcher* m, Slot& S, int n, int sw, int sh, bool settle, int memory) {
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT) fail(SLIDEO_ERR_CAPACITY, "a gated unit under SLIDEO_GATE_ANCHOR holds at most %d frames (%d)", GATE_ANCHOR_MAX_UNIT, n);
    const int64_t kp = ssd_kp((int64_t)sw * sh * 3);
    S.d_ga_a.reserve((size_t)ssd_rows_pad(n) * (size_t)kp);
    S.d_ga_rec.reserve((size_t)n * 16 + 16);
    S.d_ga_dot.reserve((size_t)n * n * 8);
    if (memory > 0) {
        S.d_gm_op.reserve((size_t)ssd_rows_pad(memory) * (size_t)kp);
        S.d_gm_rec.reserve(GM_REF_OFS + (size_t)n * 8 + 16);
        S.d_gm_dot.reserve((size_t)n * memory * 8);
        S.h_gm.reserve((size_t)n * 8);
        gate_memory_reserve_ring(m, (size_t)sw * sh * 3);
    }
    if (!settle) return;
    m->d_gate_prev.reserve((size_t)sw * sh * 3);        // (grow only from the state "none", as d_gate_small: no gated unit is reading them)
    m->d_gate_d.reserve(16);
}

void gate_memory_state_from_anchor(slideo_matcher* m, size_t sb, hipStream_t st) {
    gate_memory_reserve_ring(m, sb);
    GateMemoryMeta meta{};
    meta.ord[0] = SLIDEO_GATE_REF_RESET;
    meta.count = 1; meta.head = m->fs.gate_memory > 1 ? 1 : 0; meta.anchor = 0; meta.d = 0;
    HIP_CHECK(hipMemcpyAsync(m->d_gm_img.p, m->d_gate_small.p, sb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m->d_gm_meta.p, &meta, sizeof(meta), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));            // (meta is a stack variable)
}

// the ring's meta on the host, behind every slot's stream (a collected unit's write of the state may still be running)
static GateMemoryMeta gate_memory_read_meta(slideo_matcher* m) {
    GateMemoryMeta meta{};
    for (Slot& S : m->slots) HIP_CHECK(hipStreamSynchronize(S.st));
    HIP_CHECK(hipMemcpyAsync(&meta, m->d_gm_meta.p, sizeof(meta), hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    const int M = m->fs.gate_memory;
    if (meta.count < 1 || meta.count > M || meta.head < 0 || meta.head >= M || meta.anchor < 0 || meta.anchor >= meta.count ||
        (meta.count < M && meta.head != meta.count))
        fail(SLIDEO_ERR_HIP, "internal: gate memory ring count %d, head %d, anchor %d of %d slots", meta.count, meta.head, meta.anchor, M);
    return meta;
}

void gate_memory_read_anchor(slideo_matcher* m, size_t sb, uint8_t* out) {
    const GateMemoryMeta meta = gate_memory_read_meta(m);
    HIP_CHECK(hipMemcpyAsync(out, m->d_gm_img.as<uint8_t>() + (int64_t)meta.anchor * m->gm_stride, sb, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
}

void gate_settle_state_from_anchor(slideo_matcher* m, size_t sb, hipStream_t st) {
    m->d_gate_prev.reserve(sb);
    m->d_gate_d.reserve(16);
    HIP_CHECK(hipMemcpyAsync(m->d_gate_prev.p, m->d_gate_small.p, sb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemsetAsync(m->d_gate_d.p, 0, 4, st));
}

void gate_anchor_unit(slideo_matcher* m, Slot& S, const uint8_t* weights, const uint8_t* small, int64_t sb, int n, long long thr, long long thr_s,
                      int32_t max_defer, bool force0, hipEvent_t wait, const GateAnchorOut& out) {
    // with a gate memory the ring stands in the anchor's place ("Gate memory")
    if (m->fs.gate_memory > 0) { gate_memory_unit(m, S, weights, small, sb, n, thr, thr_s, max_defer, force0, wait, out); return; }
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

// ---- gate memory (include/slideo_amd.h "Gate memory") ------------------------------------------------------------------------------
int32_t slideo_matcher_set_gate_memory(slideo_matcher* m, int32_t capacity) {
    return matcher_set(m, SET_GATE_REFERENCE, [&](const FrameSettings& s) { return propose_gate_memory(s, capacity); });
}

int32_t slideo_matcher_gate_memory(const slideo_matcher* m, int32_t* capacity) {
    if (!m || !capacity) return SLIDEO_ERR_INVALID_ARG;
    *capacity = m->fs.gate_memory;
    return SLIDEO_OK;
}

int32_t slideo_matcher_last_gate_refs(slideo_matcher* m, int64_t* refs_out, int64_t capacity, int64_t* n) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!n) fail(SLIDEO_ERR_INVALID_ARG, "null n");
    *n = 0;
    if (m->fs.gate_memory == 0) fail(SLIDEO_ERR_STATE, "last_gate_refs: no gate memory is on (slideo_matcher_set_gate_memory)");
    if (!m->gate_refs_valid) fail(SLIDEO_ERR_STATE, "last_gate_refs: no gated call was made since the gate memory was set");
    *n = (int64_t)m->gate_refs.size();
    if (*n > 0 && (!refs_out || *n > capacity)) fail(SLIDEO_ERR_CAPACITY, "the last gated call's refs take %lld elements", (long long)*n);
    std::copy(m->gate_refs.begin(), m->gate_refs.end(), refs_out);
    API_CATCH(m)
}

int32_t slideo_matcher_gate_memory_entries(slideo_matcher* m, int32_t* count, int32_t* anchor, int64_t* ordinals_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!count || !anchor || !ordinals_out) fail(SLIDEO_ERR_INVALID_ARG, "gate_memory_entries: no null argument");
    require_idle(m);
    const int M = m->fs.gate_memory;
    if (M == 0) fail(SLIDEO_ERR_STATE, "gate_memory_entries: no gate memory is on (slideo_matcher_set_gate_memory)");
    *count = 0; *anchor = -1;
    if (!m->gate.has) return SLIDEO_OK;
    HIP_CHECK(hipSetDevice(m->device));
    const GateMemoryMeta meta = gate_memory_read_meta(m);
    // oldest first: a ring that is not full begins at slot 0, a full one at head (the slot the next match overwrites)
    const int first = meta.count < M ? 0 : meta.head;
    for (int e = 0; e < meta.count; ++e) {
        const int slot = (first + e) % M;
        ordinals_out[e] = meta.ord[slot];
        if (slot == meta.anchor) *anchor = e;
    }
    *count = meta.count;
    API_CATCH(m)
}

int32_t slideo_matcher_gate_memory_small(slideo_matcher* m, int32_t entry, uint8_t* out, int64_t capacity, int32_t* sw, int32_t* sh) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!sw || !sh) fail(SLIDEO_ERR_INVALID_ARG, "null sw/sh");
    require_idle(m);
    const int M = m->fs.gate_memory;
    if (M == 0) fail(SLIDEO_ERR_STATE, "gate_memory_small: no gate memory is on (slideo_matcher_set_gate_memory)");
    if (!m->gate.has) fail(SLIDEO_ERR_STATE, "the gate state is \"none\": no frame was gated since the last reset");
    *sw = m->gate.sw; *sh = m->gate.sh;
    HIP_CHECK(hipSetDevice(m->device));
    const GateMemoryMeta meta = gate_memory_read_meta(m);
    if (entry < 0 || entry >= meta.count) fail(SLIDEO_ERR_INVALID_ARG, "gate_memory_small: entry %d of %d", entry, meta.count);
    const int64_t sb = (int64_t)m->gate.sw * m->gate.sh * 3;
    if (!out || sb > capacity) fail(SLIDEO_ERR_CAPACITY, "small image needs %lld bytes", (long long)sb);
    const int slot = ((meta.count < M ? 0 : meta.head) + entry) % M;
    HIP_CHECK(hipMemcpyAsync(out, m->d_gm_img.as<uint8_t>() + (int64_t)slot * m->gm_stride, (size_t)sb, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    API_CATCH(m)
}

int32_t slideo_gate_recall_walk(slideo_matcher* m, const uint64_t* dot, const int64_t* norm, const uint64_t* mdot, const int64_t* mnorm,
                                const int64_t* ordinals, int32_t count, int32_t head, int32_t anchor_slot, uint64_t prev_ssd0, int32_t n, int32_t M,
                                int64_t thr_c, int64_t thr_s, int32_t max_defer, int32_t d_in, int32_t none, int64_t t0, uint8_t* changed_out,
                                uint64_t* ssd_out, int64_t* refs_out, int32_t* occupants_out, int32_t* head_out, int32_t* count_out,
                                int32_t* anchor_out, int32_t* d_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT || M < 1 || M > GATE_MEMORY_SLOTS || !dot || !norm || !mdot || !mnorm || !ordinals || !changed_out || !ssd_out ||
        !refs_out || !occupants_out || !head_out || !count_out || !anchor_out || !d_out)
        fail(SLIDEO_ERR_INVALID_ARG, "gate_recall_walk: %d frames (1 .. %d), %d slots (1 .. %d), no null argument", n, GATE_ANCHOR_MAX_UNIT, M,
             GATE_MEMORY_SLOTS);
    if (max_defer < 0 || d_in < 0 || d_in > max_defer)
        fail(SLIDEO_ERR_INVALID_ARG, "gate_recall_walk: 0 <= d_in (%d) <= max_defer (%d)", d_in, max_defer);
    // the carried ring, as the state kernel leaves it (none: nothing carried is read)
    if (!none && (count < 1 || count > M || head < 0 || head >= M || anchor_slot < 0 || anchor_slot >= count || (count < M && head != count)))
        fail(SLIDEO_ERR_INVALID_ARG, "gate_recall_walk: a ring of count %d (1 .. M = %d), head %d (count while not full), anchor slot %d (below count)",
             count, M, head, anchor_slot);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    hipStream_t st = m->slots[0].st;
    // {dot n * n | norm n | mdot n * M | mnorm M | prev_ssd0 | ssd n | ref n, twin n : 8 bytes each | meta | unit | kept list n i32, twin n,
    //  count, head 2 | flags n, twin n}
    const size_t N = (size_t)n, MM = (size_t)M;
    DevBuf d;
    d.reserve((N * N + N + N * MM + MM + 1 + 3 * N) * 8 + sizeof(GateMemoryMeta) + sizeof(GateMemoryUnit) + (2 * N + 4) * 4 + 2 * N + 16);
    unsigned long long* d_dot = d.as<unsigned long long>();
    long long* d_norm = reinterpret_cast<long long*>(d_dot + N * N);
    unsigned long long* d_mdot = reinterpret_cast<unsigned long long*>(d_norm + N);
    long long* d_mnorm = reinterpret_cast<long long*>(d_mdot + N * MM);
    unsigned long long* d_prev = reinterpret_cast<unsigned long long*>(d_mnorm + MM);
    unsigned long long* d_ssd = d_prev + 1;
    long long* d_ref = reinterpret_cast<long long*>(d_ssd + N);
    long long* d_ref2 = d_ref + N;
    GateMemoryMeta* d_meta = reinterpret_cast<GateMemoryMeta*>(d_ref2 + N);
    GateMemoryUnit* d_unit = reinterpret_cast<GateMemoryUnit*>(d_meta + 1);
    int32_t* d_idx = reinterpret_cast<int32_t*>(d_unit + 1);
    int32_t* d_idx2 = d_idx + N;
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(d_idx2 + N);
    uint32_t* d_head = d_cnt + 1;
    uint8_t* d_flag = reinterpret_cast<uint8_t*>(d_head + 3);
    uint8_t* d_flag2 = d_flag + N;
    GateMemoryMeta meta{};
    if (!none) {
        for (int c = 0; c < count; ++c) meta.ord[c] = ordinals[c];
        meta.count = count; meta.head = head; meta.anchor = anchor_slot; meta.d = (uint32_t)d_in;
    }
    const unsigned long long prev = prev_ssd0;
    HIP_CHECK(hipMemcpyAsync(d_dot, dot, N * N * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_norm, norm, N * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_mdot, mdot, N * MM * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_mnorm, mnorm, MM * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_prev, &prev, 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_meta, &meta, sizeof(meta), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));            // (meta and prev are stack variables)
    gate_recall_kernel<<<1, 64, 0, st>>>(d_dot, d_norm, d_mdot, d_mnorm, d_meta, d_prev, n, M, t0, thr_c, thr_s, (uint32_t)max_defer, none ? 1 : 0, d_flag,
                                          d_idx, d_cnt, d_head, d_ssd, d_idx2, d_flag2, d_ref, d_ref2, d_unit);
    check_launch("gate_recall_kernel");
    std::vector<uint8_t> flags(2 * N);
    std::vector<int32_t> idx(2 * N);
    std::vector<long long> refs(2 * N);
    uint32_t tail[3];                                // count, head 2
    GateMemoryUnit unit{};
    HIP_CHECK(hipMemcpyAsync(ssd_out, d_ssd, N * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(refs.data(), d_ref, 2 * N * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(flags.data(), d_flag, 2 * N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(idx.data(), d_idx, 2 * N * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(tail, d_cnt, sizeof(tail), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&unit, d_unit, sizeof(unit), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // the kernel writes everything twice (device and pinned record): the twins agree, the kept list is the flagged frames ascending
    const uint32_t cnt = tail[0];
    if (tail[1] != cnt || tail[2] != (uint32_t)n || cnt > (uint32_t)n) fail(SLIDEO_ERR_HIP, "internal: recall walk record %u / %u of %u for %d frames", cnt, tail[1], tail[2], n);
    uint32_t k = 0;
    for (size_t j = 0; j < N; ++j) {
        if (flags[j] > 1 || flags[j] != flags[N + j] || refs[j] != refs[N + j])
            fail(SLIDEO_ERR_HIP, "internal: recall walk flags / refs of frame %d: %d, %d, %lld, %lld", (int)j, (int)flags[j], (int)flags[N + j], refs[j], refs[N + j]);
        if (flags[j] && (k >= cnt || idx[k] != (int32_t)j || idx[N + k] != (int32_t)j)) fail(SLIDEO_ERR_HIP, "internal: recall walk kept list at frame %d", (int)j);
        k += flags[j];
        changed_out[j] = flags[j];
        refs_out[j] = refs[j];
    }
    if (k != cnt) fail(SLIDEO_ERR_HIP, "internal: recall walk kept %u frames, counted %u", k, cnt);
    for (int c = 0; c < GATE_MEMORY_SLOTS; ++c) occupants_out[c] = unit.occ[c];
    *head_out = unit.head; *count_out = unit.count; *anchor_out = unit.anchor; *d_out = (int32_t)unit.d;
    API_CATCH(m)
}

}  // extern "C"
