// stage_gate_anchor.hip — the gate reference SLIDEO_GATE_ANCHOR of include/slideo_amd.h "Gate reference": a gated unit's pair table
// and walk (stage_gate.hip's gate_unit_submit drives it), the setting and the tap (kernels: gate_anchor.hip.h).  The centred
// operand and the pair table are the SSD-table engine's (stage_ssd_table.hip), as the direct page look-up's are; a unit that also
// looks pages up builds the operand twice, each into its own workspace: the look-up's is made inside direct_unit_lookup, behind the
// write of the gate state.
#include "runtime.hpp"
#include "gate_anchor.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

namespace {

// S.d_ga_rec: {|a'|^2 n x i64 | SSDs against the carried anchor n x u64 | the unit's last anchor i32}
long long* ga_norm(Slot& S) { return S.d_ga_rec.as<long long>(); }
unsigned long long* ga_carried(Slot& S, int n) { return S.d_ga_rec.as<unsigned long long>() + n; }
int32_t* ga_anchor(Slot& S, int n) { return reinterpret_cast<int32_t*>(S.d_ga_rec.as<unsigned long long>() + 2 * (size_t)n); }

}  // namespace

// operand, norms and the table dot[i * n + j], i < j, of the n small images at `small` (stride sb = L bytes), on st
void gram_launch(Slot& S, const uint8_t* weights, const uint8_t* small, int64_t L, int n, hipStream_t st) {
    const int64_t kp = ssd_kp(L);
    ssd_operand_build(small, L, nullptr, n, ssd_rows_pad(n), L, kp, S.d_ga_a.as<uint4>(), ga_norm(S), st, weights);
    ssd_table_dots(S.d_ga_a.as<uint4>(), n, nullptr, n, kp, S.d_ga_dot.as<unsigned long long>(), st);
}

void gate_anchor_reserve(Slot& S, int n, int sw, int sh) {
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT) fail(SLIDEO_ERR_CAPACITY, "a gated unit under SLIDEO_GATE_ANCHOR holds at most %d frames (%d)", GATE_ANCHOR_MAX_UNIT, n);
    const int64_t kp = ssd_kp((int64_t)sw * sh * 3);
    S.d_ga_a.reserve((size_t)ssd_rows_pad(n) * (size_t)kp);
    S.d_ga_rec.reserve((size_t)n * 16 + 16);
    S.d_ga_dot.reserve((size_t)n * n * 8);
}

void gate_anchor_unit(slideo_matcher* m, Slot& S, const uint8_t* weights, const uint8_t* small, int64_t sb, int n, long long thr, bool force0,
                      hipEvent_t wait, const GateAnchorOut& out) {
    hipStream_t st = S.st;
    // every pair of the unit: nothing here reads the gate state
    gram_launch(S, weights, small, sb, n, st);
    // the carried anchor against the unit's frames, behind the previous gated unit's write of the state
    if (wait) HIP_CHECK(hipStreamWaitEvent(st, wait, 0));
    if (!force0) launch_gate_ssd(weights, m->d_gate_small.as<uint8_t>(), 0, small, sb, sb, ga_carried(S, n), n, st);
    gate_anchor_kernel<<<1, 64, 0, st>>>(S.d_ga_dot.as<unsigned long long>(), ga_norm(S), ga_carried(S, n), n, thr, force0 ? 1 : 0, out.flags, out.idx,
                                          out.count, out.h_head, out.h_ssd, out.h_idx, out.h_flag, ga_anchor(S, n));
    check_launch("gate_anchor_kernel");
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, cdiv64(sb / 4, ANCHOR_STATE_BLOCK * 4)));
    gate_anchor_state_kernel<<<blocks, ANCHOR_STATE_BLOCK, 0, st>>>(small, sb, ga_anchor(S, n), sb, m->d_gate_small.as<uint8_t>());
    check_launch("gate_anchor_state_kernel");
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
    gate_anchor_reserve(S, n, sw, sh);
    HIP_CHECK(hipMemcpyAsync(d_small.p, small, sb * n, hipMemcpyHostToDevice, st));
    gram_launch(S, weights, d_small.as<uint8_t>(), (int64_t)sb, n, st);
    std::vector<long long> norm((size_t)n);
    std::vector<unsigned long long> dot((size_t)n * n);
    HIP_CHECK(hipMemcpyAsync(norm.data(), ga_norm(S), (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(dot.data(), S.d_ga_dot.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // the table holds i < j alone: the read-out mirrors it, as gate_anchor_kernel reads one entry
    for (int i = 0; i < n; ++i) {
        ssd_out[(size_t)i * n + i] = 0;
        for (int j = i + 1; j < n; ++j) {
            const uint64_t s = (uint64_t)(norm[i] + norm[j] - 2ll * (long long)dot[(size_t)i * n + j]);
            ssd_out[(size_t)i * n + j] = s; ssd_out[(size_t)j * n + i] = s;
        }
    }
    API_CATCH(m)
}

}  // extern "C"
