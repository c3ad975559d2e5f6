// stage_gate_anchor.hip — the gate reference SLIDEO_GATE_ANCHOR of include/slideo_amd.h "Gate reference": a gated unit's pair table
// and walk (stage_gate.hip's gate_unit_submit drives it), the setting and the tap (kernels: gate_anchor.hip.h).  The centred
// operand is the direct page look-up's (stage_direct.hip launch_centre); a unit that also looks pages up builds it twice, each
// into its own workspace: the look-up's is made inside direct_unit_lookup, behind the write of the gate state.
#include "runtime.hpp"
#include "gate_anchor.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

static_assert(GRAM_TILE == DIRECT_OP_TILE && GRAM_KGRAN == DIRECT_OP_KGRAN && GRAM_KCHUNK_MAX == DIRECT_OP_KCHUNK_MAX,
              "frame_gram_kernel reads the operand of direct.hip.h");

namespace {

// S.d_ga_rec: {|a'|^2 n x i64 | SSDs against the carried anchor n x u64 | the unit's last anchor i32}
long long* ga_norm(Slot& S) { return S.d_ga_rec.as<long long>(); }
unsigned long long* ga_carried(Slot& S, int n) { return S.d_ga_rec.as<unsigned long long>() + n; }
int32_t* ga_anchor(Slot& S, int n) { return reinterpret_cast<int32_t*>(S.d_ga_rec.as<unsigned long long>() + 2 * (size_t)n); }

// operand, norms and the table dot[i * n + j], i < j, of the n small images at `small` (stride sb = L bytes), on st
void gram_launch(Slot& S, const uint8_t* weights, const uint8_t* small, int64_t L, int n, hipStream_t st) {
    const int64_t kp = direct_kp(L);
    const int n_pad = direct_rows_pad(n);
    launch_centre(small, L, nullptr, n, n_pad, L, kp, S.d_ga_a.as<uint4>(), ga_norm(S), st, weights);
    HIP_CHECK(hipMemsetAsync(S.d_ga_dot.p, 0, (size_t)n * n * 8, st));
    const int64_t kchunk = direct_kchunk(n, n, kp);
    const int64_t nz = cdiv64(kp, kchunk);
    if (kchunk > GRAM_KCHUNK_MAX || kchunk % GRAM_KGRAN || nz > 65535) fail(SLIDEO_ERR_HIP, "internal: K chunk %lld of %lld", (long long)kchunk, (long long)kp);
    const unsigned g = (unsigned)cdiv(n, 2 * GRAM_TILE);
    frame_gram_kernel<<<dim3(g, g, (unsigned)nz), GRAM_BLOCK, 0, st>>>(S.d_ga_a.as<uint4>(), n, kp, kchunk, S.d_ga_dot.as<unsigned long long>());
    check_launch("frame_gram_kernel");
}

}  // namespace

void gate_anchor_reserve(Slot& S, int n, int sw, int sh) {
    if (n < 1 || n > GATE_ANCHOR_MAX_UNIT) fail(SLIDEO_ERR_CAPACITY, "a gated unit under SLIDEO_GATE_ANCHOR holds at most %d frames (%d)", GATE_ANCHOR_MAX_UNIT, n);
    const int64_t kp = direct_kp((int64_t)sw * sh * 3);
    S.d_ga_a.reserve((size_t)direct_rows_pad(n) * (size_t)kp);
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
    const uint8_t* weights = nullptr;
    if (use_valid) {
        const GateMap& g = m->fs.gate_map;
        if (!g.on) fail(SLIDEO_ERR_STATE, "small_gram_ssd: no validity map is in force (a frame mask under SLIDEO_MASK_GATE)");
        if (sw != g.sw || sh != g.sh) fail(SLIDEO_ERR_INVALID_ARG, "small_gram_ssd: %dx%d small images, the validity map is %dx%d", sw, sh, g.sw, g.sh);
        weights = m->d_gate_w.as<uint8_t>();
    }
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
