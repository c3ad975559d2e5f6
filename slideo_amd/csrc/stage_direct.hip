// stage_direct.hip — the direct page look-up of include/slideo_amd.h "Direct page look-up": the deck's page operand (built at the
// first use), a gated unit's look-up in front of the gate's kept list (stage_gate.hip drives it), the setting and the tap
// (kernels: direct.hip.h; the operands and the table of dot products: stage_ssd_table.hip).
#include "runtime.hpp"
#include "direct.hip.h"

#include <climits>

using namespace slideo;

namespace slideo {

// gate_ssd_threshold is the smallest SSD whose similarity is < t: the largest one with >= t is the SSD in front of it
int64_t direct_ssd_threshold(float t, int64_t n) {
    const int64_t changed = gate_ssd_threshold(t, n);
    return changed == INT64_MAX ? (int64_t)255 * 255 * 3 * n : changed - 1;
}

namespace {

// The deck's size classes and their operands, on m->stream (finalized, idle matcher or the first gated unit under t > 0: nothing
// else reads or writes these buffers)
void direct_build(slideo_matcher* m) {
    if (m->direct_built) return;
    hipStream_t st = m->stream;
    const int P = (int)m->pages.size();
    std::vector<long long> small_ofs((size_t)P);
    { long long o = 0; for (int p = 0; p < P; ++p) { small_ofs[p] = o; o += (long long)m->pages[p].small_img.size(); } }
    std::vector<std::unique_ptr<DirectClass>> classes;
    for (int p = 0; p < P; ++p) {
        const HostPage& pg = m->pages[p];
        DirectClass* c = nullptr;
        for (auto& k : classes) if (k->sw == pg.sw && k->sh == pg.sh) c = k.get();
        if (!c) {
            classes.emplace_back(new DirectClass());
            c = classes.back().get();
            c->sw = pg.sw; c->sh = pg.sh; c->L = (int64_t)pg.sw * pg.sh * 3; c->kp = ssd_kp(c->L);
        }
        c->pages.push_back(p);
    }
    DevBuf d_ofs;
    for (auto& k : classes) {
        DirectClass& c = *k;
        c.np = (int)c.pages.size(); c.np_pad = ssd_rows_pad(c.np);
        std::vector<long long> ofs((size_t)c.np);
        std::vector<int32_t> all((size_t)c.np);
        for (int i = 0; i < c.np; ++i) { ofs[i] = small_ofs[c.pages[i]]; all[i] = i; }
        c.d_op.reserve((size_t)c.np_pad * (size_t)c.kp);
        c.d_norm.reserve((size_t)c.np * 8);
        c.d_pages.reserve((size_t)c.np * 4);
        c.d_all.reserve((size_t)c.np * 4);
        d_ofs.reserve((size_t)c.np * 8);
        HIP_CHECK(hipMemcpyAsync(d_ofs.p, ofs.data(), ofs.size() * 8, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(c.d_pages.p, c.pages.data(), c.pages.size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(c.d_all.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, st));
        ssd_operand_build(m->d_page_small.as<uint8_t>(), 0, d_ofs.as<long long>(), c.np, c.np_pad, c.L, c.kp, c.d_op.as<uint4>(),
                          c.d_norm.as<long long>(), st);
        HIP_CHECK(hipStreamSynchronize(st));                           // (ofs and d_ofs are reused by the next class)
    }
    m->direct_classes = std::move(classes);
    m->direct_built = true;
}

DirectClass* direct_class_for(slideo_matcher* m, int sw, int sh) {
    direct_build(m);
    for (auto& k : m->direct_classes) if (k->sw == sw && k->sh == sh) return k.get();
    return nullptr;
}

// The masked page norms of class c under the matcher's current validity map (SLIDEO_DIRECT_VALID): sum over the valid bytes of
// b'^2 per page, cached with the class under the map's generation.  On m->stream, synchronised: the map changes on an idle
// matcher only, so the unit that finds the norms stale is the only one in flight.  The deck operand is neither rebuilt nor copied.
const long long* direct_masked_norms(slideo_matcher* m, DirectClass& c) {
    const GateMap& g = m->fs.gate_map;
    if (!g.on || g.sw != c.sw || g.sh != c.sh)
        fail(SLIDEO_ERR_HIP, "internal: the gate's validity map is %dx%d (%d), the class's small images are %dx%d", g.sw, g.sh, (int)g.on, c.sw, c.sh);
    if (c.norm_v_gen == m->fs.gate_map_gen) return c.d_norm_v.as<long long>();
    hipStream_t st = m->stream;
    std::vector<long long> ofs((size_t)c.np);
    {
        std::vector<long long> small_ofs(m->pages.size());
        long long o = 0;
        for (size_t p = 0; p < m->pages.size(); ++p) { small_ofs[p] = o; o += (long long)m->pages[p].small_img.size(); }
        for (int i = 0; i < c.np; ++i) ofs[i] = small_ofs[c.pages[i]];
    }
    c.norm_v_gen = 0;
    c.d_norm_v.reserve((size_t)c.np * 8);
    DevBuf d_ofs;
    d_ofs.reserve((size_t)c.np * 8);
    HIP_CHECK(hipMemcpyAsync(d_ofs.p, ofs.data(), ofs.size() * 8, hipMemcpyHostToDevice, st));
    ssd_operand_build(m->d_page_small.as<uint8_t>(), 0, d_ofs.as<long long>(), c.np, c.np_pad, c.L, c.kp, nullptr, c.d_norm_v.as<long long>(),
                      st, m->d_gate_w.as<uint8_t>());
    HIP_CHECK(hipStreamSynchronize(st));
    c.norm_v_gen = m->fs.gate_map_gen;
    return c.d_norm_v.as<long long>();
}

// the eligible pages of `set` in class c: positions in c.pages (device, ascending) and their count
const int32_t* direct_eligible(slideo_matcher* m, const DirectClass& c, int set, int* ne) {
    if (set == 0) { *ne = c.np; return c.d_all.as<int32_t>(); }
    const auto it = m->page_sets.find(set);
    if (it == m->page_sets.end()) fail(SLIDEO_ERR_HIP, "internal: page set %d is not live", set);
    PageSet& ps = *it->second;
    for (auto& e : ps.direct_elig) if (e->cls == &c) { *ne = e->n; return e->d.as<int32_t>(); }
    std::vector<int32_t> pos;
    for (int i = 0; i < c.np; ++i) if (std::binary_search(ps.pages.begin(), ps.pages.end(), c.pages[i])) pos.push_back(i);
    std::unique_ptr<PageSet::DirectElig> e(new PageSet::DirectElig());
    e->cls = &c; e->n = (int)pos.size();
    e->d.reserve(std::max<size_t>(pos.size() * 4, 16));
    if (!pos.empty()) HIP_CHECK(hipMemcpy(e->d.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
    ps.direct_elig.push_back(std::move(e));
    *ne = ps.direct_elig.back()->n;
    return ps.direct_elig.back()->d.as<int32_t>();
}

// the slot's workspaces for n small images against class c
void direct_reserve(Slot& S, const DirectClass& c, int n) {
    S.d_dir_a.reserve((size_t)ssd_rows_pad(n) * (size_t)c.kp);
    S.d_dir_rec.reserve((size_t)n * (8 + sizeof(DirectBest)));
    S.d_dir_dot.reserve((size_t)n * c.np * 8);
}

// n small images at `small` (stride L, device) against class c: S.d_dir_a, S.d_dir_rec's norms and S.d_dir_dot (direct_reserve)
// filled on st
// (weights: the gate's validity map, the frames' operand masked; null: whole images)
void direct_dots(Slot& S, const DirectClass& c, const uint8_t* small, int n, hipStream_t st, const uint8_t* weights) {
    ssd_operand_build(small, c.L, nullptr, n, ssd_rows_pad(n), c.L, c.kp, S.d_dir_a.as<uint4>(), S.d_dir_rec.as<long long>(), st, weights);
    ssd_table_dots(S.d_dir_a.as<uint4>(), n, c.d_op.as<uint4>(), c.np, c.kp, S.d_dir_dot.as<unsigned long long>(), st);
}

DirectBest* direct_best_of(Slot& S, int n) { return reinterpret_cast<DirectBest*>(S.d_dir_rec.as<uint8_t>() + (size_t)n * 8); }

}  // namespace

DirectPlan direct_unit_prepare(slideo_matcher* m, Slot& S, int n, int sw, int sh, const uint8_t* weights) {
    DirectPlan plan;
    DirectClass* c = direct_class_for(m, sw, sh);
    if (!c) return plan;
    int ne = 0;
    const int32_t* elig = direct_eligible(m, *c, m->cur_set, &ne);
    if (ne == 0) return plan;
    direct_reserve(S, *c, n);
    plan.cls = c; plan.elig = elig; plan.ne = ne;
    plan.weights = weights;
    plan.bnorm = weights ? direct_masked_norms(m, *c) : c->d_norm.as<long long>();
    return plan;
}

void direct_unit_lookup(Slot& S, const DirectPlan& plan, int n) {
    const DirectClass* c = plan.cls;
    hipStream_t st = S.st;
    direct_dots(S, *c, S.d_gsmall.as<uint8_t>(), n, st, plan.weights);
    direct_best_kernel<<<n, DIRECT_BLOCK, 0, st>>>(S.d_dir_dot.as<unsigned long long>(), c->np, S.d_dir_rec.as<long long>(), plan.bnorm,
                                                   c->d_pages.as<int32_t>(), plan.elig, plan.ne, direct_best_of(S, n), nullptr, 0);
    check_launch("direct_best_kernel");
}

void direct_unit_gate(slideo_matcher* m, Slot& S, int n, int npx, int32_t* idx, uint32_t* count, int32_t* h_idx, uint8_t* h_rec) {
    const long long thr = direct_ssd_threshold(m->fs.direct_t, npx);
    direct_gate_kernel<<<1, DIRECT_BLOCK, 0, S.st>>>(direct_best_of(S, n), n, thr, idx, count, h_idx, h_rec);
    check_launch("direct_gate_kernel");
}

size_t direct_unit_rec_bytes(int n) { return direct_rec_bytes(n); }

uint32_t direct_rec_kept(const uint8_t* h_rec, int n) {
    const DirectHostRec r = *reinterpret_cast<const DirectHostRec*>(h_rec);
    if (r.n != (uint32_t)n || r.kept > (uint32_t)n) fail(SLIDEO_ERR_HIP, "internal: direct record %u of %u for a unit of %d", r.kept, r.n, n);
    return r.kept;
}

DirectFrameRec direct_rec_frame(const uint8_t* h_rec, int n, int i) {
    DirectFrameRec r;
    std::memcpy(&r.ssd, h_rec + direct_rec_ssd_ofs() + (size_t)i * 8, 8);
    std::memcpy(&r.page, h_rec + direct_rec_page_ofs(n) + (size_t)i * 4, 4);
    r.direct = h_rec[direct_rec_flag_ofs(n) + i] != 0;
    return r;
}

}  // namespace slideo

extern "C" {

int64_t slideo_direct_ssd_threshold(float t, int64_t n_pixels) {
    if (!(t > 0.f) || t > 1.f || n_pixels < 1 || n_pixels > INT32_MAX) return -1;
    return direct_ssd_threshold(t, n_pixels);
}

int32_t slideo_matcher_set_direct_similarity(slideo_matcher* m, float t) {
    return matcher_set(m, SET_DIRECT_SIMILARITY, [&](const FrameSettings& s) { return propose_direct_similarity(s, t); });
}

int32_t slideo_matcher_direct_similarity(const slideo_matcher* m, float* t) {
    if (!m || !t) return SLIDEO_ERR_INVALID_ARG;
    *t = m->fs.direct_t;
    return SLIDEO_OK;
}

int32_t slideo_matcher_set_direct_scope(slideo_matcher* m, uint32_t scope) {
    return matcher_set(m, SET_DIRECT_SCOPE, [&](const FrameSettings& s) { return propose_direct_scope(s, scope); });
}

int32_t slideo_matcher_direct_scope(const slideo_matcher* m, uint32_t* scope) {
    if (!m || !scope) return SLIDEO_ERR_INVALID_ARG;
    *scope = m->fs.direct_scope;
    return SLIDEO_OK;
}

// slideo_page_small_ssd (valid false) and slideo_page_small_ssd_valid (true: under the matcher's current validity map)
static void page_small_ssd_impl(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, uint64_t* ssd_out, bool valid) {
    if (!m->finalized) fail(SLIDEO_ERR_STATE, "slideo_matcher_finalize_pages must be called before the page look-up");
    if (n < 0 || sw < 1 || sh < 1 || (int64_t)sw * sh > m->cfg.small_area || (n > 0 && (!small || !ssd_out)))
        fail(SLIDEO_ERR_INVALID_ARG, "page_small_ssd: %d small images of %dx%d (at most small_area = %d pixels), small and ssd_out not null", n, sw, sh,
             m->cfg.small_area);
    const uint8_t* weights = tap_valid_weights(m, "page_small_ssd_valid", valid, sw, sh);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    if (n == 0) return;
    const int P = (int)m->pages.size();
    const size_t out_n = (size_t)n * P;
    for (size_t i = 0; i < out_n; ++i) ssd_out[i] = UINT64_MAX;
    DirectClass* c = direct_class_for(m, sw, sh);
    if (!c) return;
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    const size_t sb = (size_t)sw * sh * 3;
    DevBuf d_small, d_out;
    d_small.reserve(sb * n);
    d_out.reserve(out_n * 8);
    const long long* bnorm = weights ? direct_masked_norms(m, *c) : c->d_norm.as<long long>();
    HIP_CHECK(hipMemcpyAsync(d_small.p, small, sb * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(d_out.p, 0xFF, out_n * 8, st));
    direct_reserve(S, *c, n);
    direct_dots(S, *c, d_small.as<uint8_t>(), n, st, weights);
    direct_best_kernel<<<n, DIRECT_BLOCK, 0, st>>>(S.d_dir_dot.as<unsigned long long>(), c->np, S.d_dir_rec.as<long long>(), bnorm,
                                                   c->d_pages.as<int32_t>(), c->d_all.as<int32_t>(), c->np, direct_best_of(S, n),
                                                   d_out.as<unsigned long long>(), P);
    check_launch("direct_best_kernel");
    HIP_CHECK(hipMemcpyAsync(ssd_out, d_out.p, out_n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

int32_t slideo_page_small_ssd(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, uint64_t* ssd_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    page_small_ssd_impl(m, small, n, sw, sh, ssd_out, false);
    API_CATCH(m)
}

int32_t slideo_page_small_ssd_valid(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, uint64_t* ssd_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    page_small_ssd_impl(m, small, n, sw, sh, ssd_out, true);
    API_CATCH(m)
}

}  // extern "C"
